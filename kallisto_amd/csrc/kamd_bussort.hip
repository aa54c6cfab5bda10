// kamd_bussort.hip -- BUS records to a cells x classes matrix on the device (kamd_bus_sort, kamd_bus_count): what `bustools sort | bustools count` do
// with the records of kamd_bus_records.  The per-record rules (key digits, the plan, equality, groups) are those of kamd_bussort.h, this file is the
// sort and the compactions around them.  Neither call reads or writes the EC state, the counts, the tuple table or the fragment-length sample.
//
// kamd_bus_sort: a stable LSD radix sort over the 8-bit digits of the 24-byte key, one pass per digit in which two keys differ
//   k_sort_prep       one thread per record: the class map applied and range-checked, the record copied to the second buffer, OR and AND of the keys
//                     reduced (wavefront shuffles, then one atomicOr / atomicAnd per word and wavefront: commutative, no value is returned).  The host
//                     reads the plan and the number of bad rows: SYNCHRONISATION 1.  A bad row: error, the caller's buffer was not written.
//   per digit         k_sort_hist     a block counts the digits of its tile of SORT_TILE records -> hist[digit][block]
//                     k_bus_scan      256 blocks, one per digit: its row of block counts -> exclusive offsets, the row's total
//                     k_sort_scatter  the tile again: the digit's base (a scan of the 256 totals in LDS) + the block's offset + the record's rank in
//                                     its tile -> its place; whole records move as two 16-byte stores
//                     A wavefront owns SORT_ITEMS x 64 consecutive records of the tile and takes them 64 at a time; the rank of a record among the
//                     tile's records of its digit = the digit's count in the wavefronts before (LDS, after a barrier) + the wavefront's running count
//                     of the digit (LDS, written by one lane per digit and round) + the lanes below with the same digit (eight ballots).  No rank
//                     comes from an atomic's return value: the sort is stable and its output the same bytes on every run.
//   collapse          k_col_count / k_bus_scan / k_col_scatter: the first record of every run of equal keys is kept (flag, scan, scatter); the counts
//                     of a run are summed per wavefront segment and added to a 64-bit sum per output record (atomicAdd of integers, no value
//                     returned); k_col_final writes the sums back as counts and counts those above 32 bits.
//   The passes alternate between the caller's buffer and the second buffer; a result that ends in the second buffer is copied back.  The host reads
//   the output size and the overflow count: SYNCHRONISATION 2.
//
// kamd_bus_count (its input in key order):
//   k_cnt_heads       per record: is it out of order against its predecessor, does it begin a barcode, does it begin a (barcode, UMI) group
//   k_cnt_starts      rows: the barcodes of the barcode heads, compact; the group starts, compact, with n behind the last
//   k_cnt_mark        per record: its group g by rank; the group is multi-class when records start[g] and start[g + 1] - 1 differ in class (no thread
//                     walks a group); marks "emits a unit record" (UMIS: the head of a single-class group; READS: every record) / "goes to d_multi"
//   k_cnt_emit        unit records {row, 0, class, 1 or count, 0, row} and the multi groups' records (pad = row), both compact and in input order
//   then kamd_bus_sort's passes and collapse over the unit records (equal (row, class) of different UMIs are not adjacent in the input), and
//   k_cnt_entries     the collapsed unit records -> {row, class, value}
//   The host reads the counters behind k_cnt_emit (an unsorted input ends the call there), and the sort synchronises twice more.
// All launches are separate launches on the context stream; nothing waits for another workgroup inside a launch.
// k_cnt_heads, k_cnt_starts, k_cnt_entries and the record helpers live in kamd_bussort_dev.h, which kamd_busgenes.hip (cells x genes) includes too;
// that unit calls the sort through the kamdi functions at the end of this file.
#include "kamd_bussort_dev.h"

namespace {

constexpr int SORT_ITEMS = 4;                     // records per thread and pass
constexpr int SORT_TILE = BLOCK * SORT_ITEMS;     // records per block and pass
constexpr int SORT_WAVE_TILE = 64 * SORT_ITEMS;   // consecutive records a wavefront owns
constexpr uint8_t MARK_UNIT = 1, MARK_MULTI = 2;

// the lanes of the wavefront that are valid and hold the same digit as this one (meaningless in a lane that is not valid)
__device__ __forceinline__ u64 match_digit(u32 digit, bool valid) {
  u64 peers = __ballot(valid);
#pragma unroll
  for (int b = 0; b < 8; b++) {
    const bool bit = (digit >> b) & 1u;
    const u64 bal = __ballot(bit);
    peers &= bit ? bal : ~bal;
  }
  return peers;
}
// the tile's record this lane takes in round j: the wavefront's records in order, 64 per round
__device__ __forceinline__ u64 tile_index(int j) {
  return (u64)blockIdx.x * SORT_TILE + (u64)(threadIdx.x >> 6) * SORT_WAVE_TILE + (u64)j * 64 + (u64)lane_id();
}

__global__ __launch_bounds__(BLOCK) void k_sort_prep(const kamd_bus_record* __restrict__ in, u64 n, const int32_t* __restrict__ map, u64 n_map,
                                                     kamd_bus_record* __restrict__ out, SortCounters* ctr) {
  const u64 i = (u64)blockIdx.x * BLOCK + threadIdx.x;
  u32 o[kamd::BUS_KEY_WORDS], a[kamd::BUS_KEY_WORDS];
#pragma unroll
  for (int w = 0; w < kamd::BUS_KEY_WORDS; w++) { o[w] = 0u; a[w] = ~0u; }
  bool bad = false;
  if (i < n) {
    kamd_bus_record r = get_rec(in + i);
    if (map) {
      if (r.ec < 0 || (u64)r.ec >= n_map) bad = true;
      else r.ec = map[r.ec];
    }
    if (!bad) {
#pragma unroll
      for (int w = 0; w < kamd::BUS_KEY_WORDS; w++) o[w] = a[w] = kamd::bus_key_word(r, w);
      store_rec(out + i, q_of(r));   // (i < n: inside the second buffer of n records)
    }
  }
#pragma unroll
  for (int w = 0; w < kamd::BUS_KEY_WORDS; w++) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) { o[w] |= (u32)__shfl_xor((int)o[w], d, 64); a[w] &= (u32)__shfl_xor((int)a[w], d, 64); }
  }
  if (lane_id() == 0) {
#pragma unroll
    for (int w = 0; w < kamd::BUS_KEY_WORDS; w++) { atomicOr(&ctr->or_w[w], o[w]); atomicAnd(&ctr->and_w[w], a[w]); }
  }
  const int n_bad = __syncthreads_count(bad);
  if (threadIdx.x == 0 && n_bad) atomicAdd(&ctr->n_bad, (u64)n_bad);
}

// digit d of the record at p, from the 16-byte half that holds it
__device__ __forceinline__ u32 digit_from_half(const kamd_bus_record* p, int d) {
  const uint4 z = make_uint4(0u, 0u, 0u, 0u);
  const uint4 h = reinterpret_cast<const uint4*>(p)[d < 8 ? 1 : 0];
  RecQ x;
  x.a = d < 8 ? z : h; x.b = d < 8 ? h : z;
  return kamd::bus_key_digit(rec_of(x), d);
}

__global__ __launch_bounds__(BLOCK) void k_sort_hist(const kamd_bus_record* __restrict__ in, u64 n, int digit, u64 nb, u32* __restrict__ hist) {
  __shared__ u32 s_hist[256];
  s_hist[threadIdx.x] = 0;
  __syncthreads();
  const int lane = lane_id();
#pragma unroll
  for (int j = 0; j < SORT_ITEMS; j++) {
    const u64 idx = tile_index(j);
    const bool valid = idx < n;
    const u32 dg = valid ? digit_from_half(in + idx, digit) : 0u;
    const u64 peers = match_digit(dg, valid);
    if (valid && lane == __ffsll((unsigned long long)peers) - 1) atomicAdd(&s_hist[dg], (u32)__popcll(peers));   // (one add per digit and wavefront; the sum does not depend on their order)
  }
  __syncthreads();
  hist[(u64)threadIdx.x * nb + blockIdx.x] = s_hist[threadIdx.x];
}

// hist: the scanned rows (offset of the block among the records of a digit); tot: the rows' totals
__global__ __launch_bounds__(BLOCK) void k_sort_scatter(const kamd_bus_record* __restrict__ in, u64 n, int digit, u64 nb, const u32* __restrict__ hist,
                                                        const u64* __restrict__ tot, kamd_bus_record* __restrict__ out) {
  __shared__ u32 s_cnt[BUS_WAVES][256];   // first the wavefronts' running digit counts, then the place of a wavefront's first record of a digit
  __shared__ u32 s_w[BUS_WAVES];
  const int t = threadIdx.x, lane = lane_id(), wave = t >> 6;
#pragma unroll
  for (int w = 0; w < BUS_WAVES; w++) s_cnt[w][t] = 0;
  // where digit t begins in the output: exclusive scan of the 256 totals, plus the records of digit t in the blocks before this one
  const u32 v = (u32)tot[t];
  const u32 incl = wave_incl_scan(v);
  if (lane == 63) s_w[wave] = incl;
  __syncthreads();
  u32 base = incl - v;
  for (int w = 0; w < wave; w++) base += s_w[w];
  base += hist[(u64)t * nb + blockIdx.x];
  RecQ q[SORT_ITEMS];
  u32 dg[SORT_ITEMS], rank[SORT_ITEMS];
  volatile u32* cnt = s_cnt[wave];   // (this wavefront's row: read by every lane, then written by one lane per digit, in program order)
#pragma unroll
  for (int j = 0; j < SORT_ITEMS; j++) {
    const u64 idx = tile_index(j);
    const bool valid = idx < n;
    dg[j] = 0u; rank[j] = 0u;
    if (valid) { q[j] = load_rec(in + idx); dg[j] = kamd::bus_key_digit(rec_of(q[j]), digit); }
    const u64 peers = match_digit(dg[j], valid);
    u32 old = 0;
    if (valid) old = cnt[dg[j]];
    __builtin_amdgcn_wave_barrier();
    if (valid) {
      rank[j] = old + (u32)__popcll(peers & ((1ULL << lane) - 1ULL));
      if (lane == __ffsll((unsigned long long)peers) - 1) cnt[dg[j]] = old + (u32)__popcll(peers);
    }
    __builtin_amdgcn_wave_barrier();
  }
  __syncthreads();
  u32 run = base;
#pragma unroll
  for (int w = 0; w < BUS_WAVES; w++) { const u32 c = s_cnt[w][t]; s_cnt[w][t] = run; run += c; }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < SORT_ITEMS; j++) {
    if (tile_index(j) < n) {
      const u64 pos = (u64)s_cnt[wave][dg[j]] + rank[j];
      if (pos < n) store_rec(out + pos, q[j]);   // (a permutation of [0, n) when hist belongs to `in`; the test keeps a wrong table from leaving the buffer)
    }
  }
}

__device__ __forceinline__ bool run_head(const kamd_bus_record* rec, u64 i, u64 n, RecQ* q) {
  if (i >= n) return false;
  *q = load_rec(rec + i);
  return i == 0 || !kamd::bus_key_equal(get_rec(rec + i - 1), rec_of(*q));
}

__global__ __launch_bounds__(BLOCK) void k_col_count(const kamd_bus_record* __restrict__ in, u64 n, u32* __restrict__ blk_cnt) {
  const u64 i = (u64)blockIdx.x * BLOCK + threadIdx.x;
  RecQ q;
  const int heads = __syncthreads_count(run_head(in, i, n, &q));
  if (threadIdx.x == 0) blk_cnt[blockIdx.x] = (u32)heads;
}

__global__ __launch_bounds__(BLOCK) void k_col_scatter(const kamd_bus_record* __restrict__ in, u64 n, const u32* __restrict__ blk_off,
                                                       kamd_bus_record* __restrict__ out, u64* __restrict__ sum) {
  __shared__ u32 s_w[BUS_WAVES];
  const u64 i = (u64)blockIdx.x * BLOCK + threadIdx.x;
  const int lane = lane_id();
  RecQ q;
  const bool head = run_head(in, i, n, &q);
  const u32 before = block_rank(head, s_w);
  // the run of record i is output record j (record 0 is a head: j >= 0; j < the number of heads <= n)
  const u32 j = i < n ? blk_off[blockIdx.x] + before + (head ? 1u : 0u) - 1u : 0xFFFFFFFFu;
  if (head) store_rec(out + j, q);
  // the counts of a run, summed over the lanes of the wavefront that hold it (consecutive lanes: j ascends with the lane)
  u64 v = i < n ? (u64)q.b.y : 0ULL;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const u64 tv = ((u64)(u32)__shfl_up((int)(v >> 32), d, 64) << 32) | (u32)__shfl_up((int)v, d, 64);
    const u32 tj = (u32)__shfl_up((int)j, d, 64);
    if (lane >= d && tj == j) v += tv;
  }
  const u32 nj = (u32)__shfl_down((int)j, 1, 64);
  if (i < n && (lane == 63 || nj != j)) atomicAdd(&sum[j], v);   // (integer adds: the sum does not depend on their order)
}

__global__ __launch_bounds__(BLOCK) void k_col_final(kamd_bus_record* __restrict__ out, const u64* __restrict__ sum, SortCounters* ctr) {
  const u64 j = (u64)blockIdx.x * BLOCK + threadIdx.x;
  bool over = false;
  if (j < ctr->n_out) {
    const u64 s = sum[j];
    over = s > 0xFFFFFFFFULL;
    if (!over) out[j].count = (u32)s;
  }
  const int n_over = __syncthreads_count(over);
  if (threadIdx.x == 0 && n_over) atomicAdd(&ctr->n_over, (u64)n_over);
}


__global__ __launch_bounds__(BLOCK) void k_cnt_mark(const kamd_bus_record* __restrict__ rec, u64 n, int mode, const u32* __restrict__ blk_grp, const u32* __restrict__ gstart,
                                                    SortCounters* ctr, uint8_t* __restrict__ mark, u32* __restrict__ blk_unit, u32* __restrict__ blk_multi) {
  __shared__ u32 s_w[BUS_WAVES];
  if (ctr->n_unsorted) return;   // (uniform)
  const u64 i = (u64)blockIdx.x * BLOCK + threadIdx.x;
  kamd_bus_record me;
  const Heads h = rec_heads(rec, i, n, &me);
  const u32 before = block_rank(h.grp, s_w);
  bool unit = false, multi = false;
  if (i < n) {
    if (mode == KAMD_BUS_COUNT_READS) unit = true;
    else {
      const u64 g = (u64)blk_grp[blockIdx.x] + before + (h.grp ? 1u : 0u) - 1u;   // (record 0 begins group 0; g < n_groups)
      const u64 first = gstart[g], last = (u64)gstart[g + 1] - 1;                // (first <= i <= last < n)
      multi = kamd::bus_group_multi(get_rec(rec + first), get_rec(rec + last));
      unit = h.grp && !multi;
    }
    mark[i] = (uint8_t)((unit ? MARK_UNIT : 0) | (multi ? MARK_MULTI : 0));
  }
  const int n_unit = __syncthreads_count(unit), n_multi = __syncthreads_count(multi), n_mgrp = __syncthreads_count(multi && h.grp);
  if (threadIdx.x == 0) {
    blk_unit[blockIdx.x] = (u32)n_unit;
    blk_multi[blockIdx.x] = (u32)n_multi;
    if (n_mgrp) atomicAdd(&ctr->n_multi_grp, (u64)n_mgrp);
  }
}

__global__ __launch_bounds__(BLOCK) void k_cnt_emit(const kamd_bus_record* __restrict__ rec, u64 n, int mode, const uint8_t* __restrict__ mark, const u32* __restrict__ blk_bc,
                                                    const u32* __restrict__ blk_unit, const u32* __restrict__ blk_multi, const SortCounters* __restrict__ ctr,
                                                    kamd_bus_record* __restrict__ units, kamd_bus_record* __restrict__ multi_out) {
  __shared__ u32 s_w[3][BUS_WAVES];
  if (ctr->n_unsorted) return;   // (uniform)
  const u64 i = (u64)blockIdx.x * BLOCK + threadIdx.x;
  kamd_bus_record me;
  const Heads h = rec_heads(rec, i, n, &me);
  const uint8_t m = i < n ? mark[i] : (uint8_t)0;
  const u32 r_bc = block_rank(h.bc, s_w[0]), r_unit = block_rank(m & MARK_UNIT, s_w[1]), r_multi = block_rank(m & MARK_MULTI, s_w[2]);
  if (i >= n) return;
  const u32 row = blk_bc[blockIdx.x] + r_bc + (h.bc ? 1u : 0u) - 1u;
  if (m & MARK_UNIT) store_rec(units + ((u64)blk_unit[blockIdx.x] + r_unit), q_of(kamd::bus_unit_record(me, row, mode)));   // (compact: inside [n])
  if (m & MARK_MULTI) { me.pad = row; store_rec(multi_out + ((u64)blk_multi[blockIdx.x] + r_multi), q_of(me)); }
}


int read_counters(kamd_ctx* c, SortCounters* h) {
  HIPC(hipGetLastError());
  HIPC(hipMemcpyAsync(h, c->bsort_ctr.p, sizeof *h, hipMemcpyDeviceToHost, c->stream));
  HIPC(hipStreamSynchronize(c->stream));
  return 0;
}

// the sort of both entry points; `who` begins the error texts.  Two host synchronisations: the plan, and the output size at the end
int sort_records(kamd_ctx* c, kamd_bus_record* d_rec, u64 n, const int32_t* d_map, u64 n_map, int collapse, u64* n_out, kamd_bus_sort_stats* st, const std::string& who) {
  const u64 nb = grid_for(n, SORT_TILE), nb1 = grid_for(n, BLOCK);
  if (int rc = c->bsort_b.ensure(n * sizeof(kamd_bus_record), 0, c->stream)) return rc;
  if (int rc = c->bsort_hist.ensure(256 * nb * sizeof(u32), 0, c->stream)) return rc;
  if (int rc = c->bsort_tot.ensure(256 * sizeof(u64), 0, c->stream)) return rc;
  if (int rc = c->bsort_ctr.ensure(sizeof(SortCounters), 0, c->stream)) return rc;
  if (int rc = c->bus_blk.ensure(nb1 * sizeof(u32), 0, c->stream)) return rc;
  if (collapse) if (int rc = c->bsort_sum.ensure(n * sizeof(u64), 0, c->stream)) return rc;
  SortCounters* ctr = c->bsort_ctr.as<SortCounters>();
  HIPC(hipMemsetAsync(ctr, 0, sizeof *ctr, c->stream));
  HIPC(hipMemsetAsync(ctr->and_w, 0xFF, sizeof ctr->and_w, c->stream));
  kamd_bus_record *a = d_rec, *b = c->bsort_b.as<kamd_bus_record>();
  hipLaunchKernelGGL(k_sort_prep, dim3((unsigned)nb1), dim3(BLOCK), 0, c->stream, (const kamd_bus_record*)a, n, d_map, n_map, b, ctr);
  SortCounters h{};
  if (int rc = read_counters(c, &h)) return rc;   // synchronisation 1: the plan
  if (h.n_bad)
    return kamd::fail(-4, who + ": " + std::to_string(h.n_bad) + " records name a class outside the map's [0, " + std::to_string(n_map) + "); nothing written");
  const uint32_t plan = kamd::bus_sort_plan(reinterpret_cast<const uint8_t*>(h.or_w), reinterpret_cast<const uint8_t*>(h.and_w));
  uint32_t passes = 0, key_bits = 0;
  for (int w = 0; w < kamd::BUS_KEY_WORDS; w++) key_bits += (uint32_t)__builtin_popcount(h.or_w[w] ^ h.and_w[w]);
  kamd_bus_record *src = b, *dst = a;
  u32* hist = c->bsort_hist.as<u32>();
  u64* tot = c->bsort_tot.as<u64>();
  for (int d = 0; d < kamd::BUS_KEY_DIGITS; d++) {
    if (!((plan >> d) & 1u)) continue;
    hipLaunchKernelGGL(k_sort_hist, dim3((unsigned)nb), dim3(BLOCK), 0, c->stream, (const kamd_bus_record*)src, n, d, nb, hist);
    hipLaunchKernelGGL(k_bus_scan, dim3(256), dim3(BLOCK), 0, c->stream, hist, nb, tot);
    hipLaunchKernelGGL(k_sort_scatter, dim3((unsigned)nb), dim3(BLOCK), 0, c->stream, (const kamd_bus_record*)src, n, d, nb, (const u32*)hist, (const u64*)tot, dst);
    std::swap(src, dst);
    ++passes;
  }
  if (collapse) {
    u32* blk = c->bus_blk.as<u32>();
    u64* sum = c->bsort_sum.as<u64>();
    HIPC(hipMemsetAsync(sum, 0, n * sizeof(u64), c->stream));
    hipLaunchKernelGGL(k_col_count, dim3((unsigned)nb1), dim3(BLOCK), 0, c->stream, (const kamd_bus_record*)src, n, blk);
    hipLaunchKernelGGL(k_bus_scan, dim3(1), dim3(BLOCK), 0, c->stream, blk, nb1, &ctr->n_out);
    hipLaunchKernelGGL(k_col_scatter, dim3((unsigned)nb1), dim3(BLOCK), 0, c->stream, (const kamd_bus_record*)src, n, (const u32*)blk, dst, sum);
    hipLaunchKernelGGL(k_col_final, dim3((unsigned)nb1), dim3(BLOCK), 0, c->stream, dst, (const u64*)sum, ctr);
    std::swap(src, dst);
  }
  if (src != a) HIPC(hipMemcpyAsync(a, src, n * sizeof(kamd_bus_record), hipMemcpyDeviceToDevice, c->stream));
  if (int rc = read_counters(c, &h)) return rc;   // synchronisation 2: the output size
  if (h.n_over)
    return kamd::fail(-4, who + ": the counts of " + std::to_string(h.n_over) + " collapsed records sum to more than 0xFFFFFFFF");
  *n_out = collapse ? h.n_out : n;
  if (st) { st->n_in = n; st->n_out = *n_out; st->passes = passes; st->key_bits = key_bits; }
  return 0;
}

int events_begin(kamd_ctx* c) {
  HIPC(hipSetDevice(c->device));
  for (hipEvent_t& e : c->bus_ev) if (!e) HIPC(hipEventCreate(&e));
  HIPC(hipEventRecord(c->bus_ev[0], c->stream));
  return 0;
}
int events_end(kamd_ctx* c, float* ms) {
  HIPC(hipEventRecord(c->bus_ev[1], c->stream));
  HIPC(hipEventSynchronize(c->bus_ev[1]));
  HIPC(hipEventElapsedTime(ms, c->bus_ev[0], c->bus_ev[1]));
  return 0;
}
bool misaligned(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) != 0; }

}  // namespace

namespace kamdi {   // (what kamd_busgenes.hip calls: kamd_bussort_dev.h)
int bus_sort_records(kamd_ctx* c, kamd_bus_record* d_rec, u64 n, const int32_t* d_map, u64 n_map, int collapse, u64* n_out, kamd_bus_sort_stats* st, const std::string& who) {
  return sort_records(c, d_rec, n, d_map, n_map, collapse, n_out, st, who);
}
int bus_read_counters(kamd_ctx* c, SortCounters* h) { return read_counters(c, h); }
int bus_events_begin(kamd_ctx* c) { return events_begin(c); }
int bus_events_end(kamd_ctx* c, float* ms) { return events_end(c, ms); }
}  // namespace kamdi

extern "C" int kamd_bus_sort(kamd_ctx* c, kamd_bus_record* d_rec, uint64_t n, const int32_t* d_ec_map, uint64_t n_map, int collapse, uint64_t* n_out,
                             kamd_bus_sort_stats* out) {
  if (!c || !n_out) return kamd::fail(-1, "kamd_bus_sort: null argument");
  *n_out = 0;
  if (out) memset(out, 0, sizeof *out);
  if (n >= 0xFFFFFFFFULL) return kamd::fail(-1, "kamd_bus_sort: a call takes fewer than 2^32 - 1 records");
  if (n == 0) return 0;
  if (!d_rec) return kamd::fail(-1, "kamd_bus_sort: null argument");
  if (misaligned(d_rec)) return kamd::fail(-1, "kamd_bus_sort: the records must be 16-byte aligned");
  if (int rc = events_begin(c)) return rc;
  u64 kept = 0;
  if (int rc = sort_records(c, d_rec, n, d_ec_map, d_ec_map ? n_map : 0, collapse, &kept, out, "kamd_bus_sort")) return rc;
  *n_out = kept;
  float ms = 0.f;
  if (int rc = events_end(c, &ms)) return rc;
  if (out) out->last_ms = ms;
  return 0;
}

extern "C" int kamd_bus_count(kamd_ctx* c, const kamd_bus_record* d_sorted, uint64_t n, int mode, uint64_t* d_barcodes, kamd_bus_entry* d_entries,
                              kamd_bus_record* d_multi, kamd_bus_count_stats* out) {
  if (!c) return kamd::fail(-1, "kamd_bus_count: null context");
  if (out) memset(out, 0, sizeof *out);
  if (mode != KAMD_BUS_COUNT_UMIS && mode != KAMD_BUS_COUNT_READS) return kamd::fail(-1, "kamd_bus_count: mode must be KAMD_BUS_COUNT_UMIS or KAMD_BUS_COUNT_READS");
  if (n >= 0xFFFFFFFFULL) return kamd::fail(-1, "kamd_bus_count: a call takes fewer than 2^32 - 1 records");
  if (n == 0) return 0;
  if (!d_sorted || !d_barcodes || !d_entries || !d_multi) return kamd::fail(-1, "kamd_bus_count: null argument");
  if (misaligned(d_sorted) || misaligned(d_multi)) return kamd::fail(-1, "kamd_bus_count: the records must be 16-byte aligned");
  if (int rc = events_begin(c)) return rc;
  const u64 nb = grid_for(n, BLOCK);
  if (int rc = c->bcnt_blk.ensure(4 * nb * sizeof(u32), 0, c->stream)) return rc;
  if (int rc = c->bcnt_units.ensure(n * sizeof(kamd_bus_record), 0, c->stream)) return rc;
  if (int rc = c->bcnt_gstart.ensure((n + 1) * sizeof(u32), 0, c->stream)) return rc;
  if (int rc = c->bcnt_mark.ensure(n, 0, c->stream)) return rc;
  if (int rc = c->bsort_ctr.ensure(sizeof(SortCounters), 0, c->stream)) return rc;
  SortCounters* ctr = c->bsort_ctr.as<SortCounters>();
  HIPC(hipMemsetAsync(ctr, 0, sizeof *ctr, c->stream));
  u32 *blk_bc = c->bcnt_blk.as<u32>(), *blk_grp = blk_bc + nb, *blk_unit = blk_grp + nb, *blk_multi = blk_unit + nb;
  kamd_bus_record* units = c->bcnt_units.as<kamd_bus_record>();
  u32* gstart = c->bcnt_gstart.as<u32>();
  uint8_t* mark = c->bcnt_mark.as<uint8_t>();
  const dim3 g((unsigned)nb), t(BLOCK);
  hipLaunchKernelGGL(k_cnt_heads, g, t, 0, c->stream, d_sorted, (u64)n, blk_bc, blk_grp, ctr);
  hipLaunchKernelGGL(k_bus_scan, dim3(1), t, 0, c->stream, blk_bc, nb, &ctr->n_barcodes);
  hipLaunchKernelGGL(k_bus_scan, dim3(1), t, 0, c->stream, blk_grp, nb, &ctr->n_groups);
  hipLaunchKernelGGL(k_cnt_starts, g, t, 0, c->stream, d_sorted, (u64)n, (const u32*)blk_bc, (const u32*)blk_grp, (const SortCounters*)ctr, (u64*)d_barcodes, gstart);
  hipLaunchKernelGGL(k_cnt_mark, g, t, 0, c->stream, d_sorted, (u64)n, mode, (const u32*)blk_grp, (const u32*)gstart, ctr, mark, blk_unit, blk_multi);
  hipLaunchKernelGGL(k_bus_scan, dim3(1), t, 0, c->stream, blk_unit, nb, &ctr->n_units);
  hipLaunchKernelGGL(k_bus_scan, dim3(1), t, 0, c->stream, blk_multi, nb, &ctr->n_multi_rec);
  hipLaunchKernelGGL(k_cnt_emit, g, t, 0, c->stream, d_sorted, (u64)n, mode, (const uint8_t*)mark, (const u32*)blk_bc, (const u32*)blk_unit, (const u32*)blk_multi,
                     (const SortCounters*)ctr, units, d_multi);
  SortCounters h{};
  if (int rc = read_counters(c, &h)) return rc;   // (the sort below starts its own counters: these are read first)
  if (h.n_unsorted)
    return kamd::fail(-4, "kamd_bus_count: " + std::to_string(h.n_unsorted) + " records lie before their predecessor in key order: the input is not sorted; nothing counted");
  u64 n_entries = 0;
  if (h.n_units) {
    if (int rc = sort_records(c, units, h.n_units, nullptr, 0, 1, &n_entries, nullptr, "kamd_bus_count")) return rc;
    hipLaunchKernelGGL(k_cnt_entries, dim3(grid_for(n_entries, BLOCK)), t, 0, c->stream, (const kamd_bus_record*)units, n_entries, d_entries);
    HIPC(hipGetLastError());
  }
  float ms = 0.f;
  if (int rc = events_end(c, &ms)) return rc;
  if (out) {
    out->n_records = n; out->n_barcodes = h.n_barcodes; out->n_entries = n_entries; out->n_umis = h.n_groups;
    out->n_multi_groups = h.n_multi_grp; out->n_multi_records = h.n_multi_rec; out->last_ms = ms;
  }
  return 0;
}
