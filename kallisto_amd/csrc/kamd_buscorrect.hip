// kamd_buscorrect.hip -- barcode whitelists on the device (kamd_bus_whitelist_create, kamd_bus_correct): what `bustools correct` does with the records
// of kamd_bus_records before kamd_bus_sort takes them.  The table's layout, the hash, the neighbours and the status rule are those of
// kamd_buscorrect.h; this file is the kernels around them.  Neither call reads or writes the EC state, the counts, the tuple table or the
// fragment-length sample.
//
// kamd_bus_whitelist_create: the codes are checked on the host (bits above 2 L, the marker value at L = 32), uploaded, and
//   k_wl_insert       one thread per key: the first empty slot from the home bucket on is claimed with a 64-bit atomicCAS; a returned value equal to
//                     the key is a duplicate.  Which slot a key gets depends on the order of the threads, whether a key is found does not: a walk
//                     for a key passes only slots that were taken before the key's own.  The claimed slots are counted (n_distinct), the longest
//                     walk is kept with atomicMax (max_chain).
// kamd_bus_correct:
//   k_cor_exact       one thread per record: the home bucket as four 16-byte loads (and the buckets behind it while they are full).  Status EXACT, or
//                     UNCORRECTABLE for a barcode with high bits, is final; any other record's index goes to the miss list: ranks by ballot within
//                     the block, the block's place in the list by one atomicAdd (the list's order varies from run to run; nothing is derived from it)
//   k_cor_neigh       one wavefront per missed record, lane j tests neighbour j: ceil(3 L / 64) rounds, one for L <= 21, two beyond.  The ballots of
//                     the hits are counted; at exactly one the hitting lane writes the barcode the record takes, lane 0 the status.  The grid is
//                     fixed (the length of the list stays on the device), a wavefront takes every gridDim.x * 4-th miss.
//   k_cor_count / k_bus_scan / k_cor_scatter   the records with status <= 1, compact and in input order; the scatter puts the corrected barcode in
//                     place.  k_cor_count also sums the four statuses (integer adds, no value returned).
//   The host reads the counters: the call's one synchronisation.
// All launches are separate launches on the context stream; nothing waits for another workgroup inside a launch.
#include "kamd_dev.h"
#include "kamd_buscorrect.h"
#include "kamd_bus_scan.h"

struct kamd_bus_whitelist {
  u64* slots = nullptr;
  u64 n_buckets = 0;
  int32_t bc_len = 0, has_marker = 0;
  kamd_bus_whitelist_stats stats{};
};

namespace {

constexpr int WAVES = BLOCK / 64;

struct WlCounters { u64 n_distinct, n_fail; u32 max_chain, pad; };
struct CorCounters { u64 n_miss, n_status[4], n_out; };

__device__ __forceinline__ u64 u64_of(u32 lo, u32 hi) { return (u64)lo | ((u64)hi << 32); }

// membership on the device: a bucket is one 64-byte line, read as four 16-byte loads
__device__ __forceinline__ bool dev_contains(const kamd::WlTable& t, u64 key) {
  return kamd::wl_contains_with(t, (uint64_t)key, [&](uint64_t b, uint64_t* k) {
    const uint4* q = reinterpret_cast<const uint4*>(t.slots + b * kamd::WL_BUCKET_KEYS);   // (b < n_buckets: masked by the caller)
    const uint4 v0 = q[0], v1 = q[1], v2 = q[2], v3 = q[3];
    k[0] = u64_of(v0.x, v0.y); k[1] = u64_of(v0.z, v0.w); k[2] = u64_of(v1.x, v1.y); k[3] = u64_of(v1.z, v1.w);
    k[4] = u64_of(v2.x, v2.y); k[5] = u64_of(v2.z, v2.w); k[6] = u64_of(v3.x, v3.y); k[7] = u64_of(v3.z, v3.w);
  });
}

__global__ __launch_bounds__(BLOCK) void k_wl_insert(const u64* __restrict__ codes, u64 n, u64* slots, u64 n_buckets, WlCounters* ctr) {
  const u64 i = (u64)blockIdx.x * BLOCK + threadIdx.x;
  bool is_new = false, fail = false;
  u32 chain = 0;
  if (i < n) {
    const u64 key = codes[i];
    if (key != kamd::WL_EMPTY) {   // (the marker value is a flag of the whitelist, not a slot)
      chain = kamd::wl_insert((uint64_t*)slots, (uint64_t)n_buckets, (uint64_t)key, &is_new,
                              [](uint64_t* p, uint64_t expect, uint64_t want) { return (uint64_t)atomicCAS((u64*)p, (u64)expect, (u64)want); });
      fail = chain == 0;
    }
  }
  u32 mx = chain;
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) mx = max(mx, (u32)__shfl_xor((int)mx, d, 64));
  if (lane_id() == 0 && mx) atomicMax(&ctr->max_chain, mx);
  const int n_new = __syncthreads_count(is_new), n_fail = __syncthreads_count(fail);
  if (threadIdx.x == 0) {
    if (n_new) atomicAdd(&ctr->n_distinct, (u64)n_new);
    if (n_fail) atomicAdd(&ctr->n_fail, (u64)n_fail);
  }
}

__global__ __launch_bounds__(BLOCK) void k_cor_exact(kamd::WlTable t, const kamd_bus_record* __restrict__ in, u64 n, uint8_t* __restrict__ status,
                                                     u32* __restrict__ miss, CorCounters* ctr) {
  __shared__ u32 s_w[BUS_WAVES];
  __shared__ u32 s_base;
  const u64 i = (u64)blockIdx.x * BLOCK + threadIdx.x;
  bool missed = false;
  if (i < n) {
    const u64 b = in[i].barcode;
    if (b & kamd::wl_high_mask(t.bc_len)) status[i] = KAMD_BUS_COR_UNCORRECTABLE;
    else if (dev_contains(t, b)) status[i] = KAMD_BUS_COR_EXACT;
    else missed = true;   // (its status is k_cor_neigh's to write)
  }
  const u32 rank = block_rank(missed, s_w);
  if (threadIdx.x == 0) {
    u32 cnt = 0;
    for (int w = 0; w < BUS_WAVES; w++) cnt += s_w[w];
    s_base = cnt ? (u32)atomicAdd(&ctr->n_miss, (u64)cnt) : 0u;
  }
  __syncthreads();
  if (missed) {
    const u64 at = (u64)s_base + rank;
    if (at < n) miss[at] = (u32)i;   // (the blocks' counts sum to at most n: inside the list of n entries)
  }
}

__global__ __launch_bounds__(BLOCK) void k_cor_neigh(kamd::WlTable t, const kamd_bus_record* __restrict__ in, u64 n, const u32* __restrict__ miss,
                                                     const CorCounters* __restrict__ ctr, uint8_t* __restrict__ status, u64* __restrict__ fix) {
  const int lane = lane_id();
  const u64 n_miss = min(ctr->n_miss, n), stride = (u64)gridDim.x * WAVES;
  const int n_nb = 3 * t.bc_len;
  for (u64 m = (u64)blockIdx.x * WAVES + (threadIdx.x >> 6); m < n_miss; m += stride) {   // (uniform over the wavefront)
    const u64 i = miss[m];
    if (i >= n) continue;
    const u64 b = in[i].barcode;
    u32 total = 0;
    u64 mine = 0;
    bool mine_hit = false;
    for (int j0 = 0; j0 < n_nb; j0 += 64) {
      const int j = j0 + lane;
      bool hit = false;
      u64 nb = 0;
      if (j < n_nb) { nb = kamd::wl_neighbour(b, t.bc_len, j); hit = dev_contains(t, nb); }
      total += (u32)__popcll(__ballot(hit));
      if (hit) { mine = nb; mine_hit = true; }
    }
    if (total == 1 && mine_hit) fix[i] = mine;
    if (lane == 0) status[i] = (uint8_t)kamd::wl_miss_status(total);
  }
}

__global__ __launch_bounds__(BLOCK) void k_cor_count(const uint8_t* __restrict__ status, u64 n, u32* __restrict__ blk_cnt, CorCounters* ctr) {
  const u64 i = (u64)blockIdx.x * BLOCK + threadIdx.x;
  const int s = i < n ? (int)status[i] : -1;
  int c[4];
#pragma unroll
  for (int k = 0; k < 4; k++) c[k] = __syncthreads_count(s == k);
  if (threadIdx.x == 0) {
    blk_cnt[blockIdx.x] = (u32)(c[0] + c[1]);
#pragma unroll
    for (int k = 0; k < 4; k++) if (c[k]) atomicAdd(&ctr->n_status[k], (u64)c[k]);
  }
}

__global__ __launch_bounds__(BLOCK) void k_cor_scatter(const kamd_bus_record* __restrict__ in, u64 n, const uint8_t* __restrict__ status, const u64* __restrict__ fix,
                                                       const u32* __restrict__ blk_off, kamd_bus_record* __restrict__ out) {
  __shared__ u32 s_w[BUS_WAVES];
  const u64 i = (u64)blockIdx.x * BLOCK + threadIdx.x;
  const int s = i < n ? (int)status[i] : 3;
  const bool keep = s <= KAMD_BUS_COR_CORRECTED;
  const u32 rank = block_rank(keep, s_w);
  if (!keep) return;
  const uint4* q = reinterpret_cast<const uint4*>(in + i);
  uint4 a = q[0];
  const uint4 b = q[1];
  if (s == KAMD_BUS_COR_CORRECTED) { const u64 f = fix[i]; a.x = (u32)f; a.y = (u32)(f >> 32); }
  const u64 pos = (u64)blk_off[blockIdx.x] + rank;   // (the survivors before this one: pos <= i < n)
  uint4* o = reinterpret_cast<uint4*>(out + pos);
  o[0] = a; o[1] = b;
}

bool misaligned(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) != 0; }

int events_ready(kamd_ctx* c) {
  HIPC(hipSetDevice(c->device));
  for (hipEvent_t& e : c->bus_ev) if (!e) HIPC(hipEventCreate(&e));
  for (hipEvent_t& e : c->bcor_ev) if (!e) HIPC(hipEventCreate(&e));
  return 0;
}

bool owns(const kamd_ctx* c, const kamd_bus_whitelist* wl) { return std::find(c->whitelists.begin(), c->whitelists.end(), wl) != c->whitelists.end(); }

}  // namespace

namespace kamdi {
void whitelists_free_all(kamd_ctx* c) {
  for (kamd_bus_whitelist* wl : c->whitelists) {
    if (wl->slots) (void)hipFree(wl->slots);
    delete wl;
  }
  c->whitelists.clear();
}
}  // namespace kamdi

extern "C" int kamd_bus_whitelist_create(kamd_ctx* c, const uint64_t* h_codes, uint64_t n, int32_t bc_len, kamd_bus_whitelist** out, kamd_bus_whitelist_stats* stats) {
  if (out) *out = nullptr;
  if (stats) memset(stats, 0, sizeof *stats);
  if (!c || !out) return kamd::fail(-1, "kamd_bus_whitelist_create: null argument");
  if (bc_len < 1 || bc_len > 32) return kamd::fail(-1, "kamd_bus_whitelist_create: the barcode length must be in [1, 32], not " + std::to_string(bc_len));
  if (n == 0) return kamd::fail(-1, "kamd_bus_whitelist_create: an empty whitelist");
  if (n >= 0xFFFFFFFFULL) return kamd::fail(-1, "kamd_bus_whitelist_create: a whitelist holds fewer than 2^32 - 1 barcodes");
  if (!h_codes) return kamd::fail(-1, "kamd_bus_whitelist_create: null argument");
  const u64 high = kamd::wl_high_mask(bc_len);
  int32_t has_marker = 0;
  for (u64 i = 0; i < n; i++) {
    if (h_codes[i] & high)
      return kamd::fail(-1, "kamd_bus_whitelist_create: code " + std::to_string(i) + " has a bit set above bit " + std::to_string(2 * bc_len - 1) + ": no barcode of " +
                                std::to_string(bc_len) + " bases");
    if (h_codes[i] == kamd::WL_EMPTY) has_marker = 1;   // (bc_len == 32: 32 T)
  }
  if (int rc = events_ready(c)) return rc;
  const u64 n_buckets = kamd::wl_n_buckets(n), bytes = n_buckets * kamd::WL_BUCKET_KEYS * sizeof(u64);
  if (int rc = c->bcor_ctr.ensure(std::max(sizeof(WlCounters), sizeof(CorCounters)), 0, c->stream)) return rc;
  u64 *slots = nullptr, *d_codes = nullptr;
  HIPC(hipMalloc((void**)&slots, bytes));
  if (hipMalloc((void**)&d_codes, n * sizeof(u64)) != hipSuccess) { (void)hipFree(slots); return kamd::fail(-100, "kamd_bus_whitelist_create: hipMalloc of the codes failed"); }
  WlCounters* ctr = c->bcor_ctr.as<WlCounters>();
  WlCounters h{};
  float ms = 0.f;
  auto run = [&]() -> int {
    HIPC(hipEventRecord(c->bus_ev[0], c->stream));
    HIPC(hipMemsetAsync(slots, 0xFF, bytes, c->stream));
    HIPC(hipMemsetAsync(ctr, 0, sizeof *ctr, c->stream));
    HIPC(hipMemcpyAsync(d_codes, h_codes, n * sizeof(u64), hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(k_wl_insert, dim3(grid_for(n, BLOCK)), dim3(BLOCK), 0, c->stream, (const u64*)d_codes, (u64)n, slots, n_buckets, ctr);
    HIPC(hipGetLastError());
    HIPC(hipEventRecord(c->bus_ev[1], c->stream));
    HIPC(hipMemcpyAsync(&h, ctr, sizeof h, hipMemcpyDeviceToHost, c->stream));
    HIPC(hipStreamSynchronize(c->stream));
    HIPC(hipEventElapsedTime(&ms, c->bus_ev[0], c->bus_ev[1]));
    return 0;
  };
  const int rc = run();
  (void)hipFree(d_codes);
  if (rc || h.n_fail) {
    (void)hipFree(slots);
    return rc ? rc : kamd::fail(-4, "kamd_bus_whitelist_create: " + std::to_string(h.n_fail) + " barcodes found no slot");
  }
  kamd_bus_whitelist* wl = new kamd_bus_whitelist;
  wl->slots = slots; wl->n_buckets = n_buckets; wl->bc_len = bc_len; wl->has_marker = has_marker;
  wl->stats.n_in = n; wl->stats.n_distinct = h.n_distinct + (u64)has_marker; wl->stats.n_buckets = n_buckets; wl->stats.bytes = bytes;
  wl->stats.max_chain = h.max_chain; wl->stats.bc_len = bc_len; wl->stats.last_ms = ms;
  c->whitelists.push_back(wl);
  if (stats) *stats = wl->stats;
  *out = wl;
  return 0;
}

extern "C" int kamd_bus_whitelist_free(kamd_ctx* c, kamd_bus_whitelist* wl) {
  if (!c) return kamd::fail(-1, "kamd_bus_whitelist_free: null context");
  if (!wl) return 0;
  if (!owns(c, wl)) return kamd::fail(-1, "kamd_bus_whitelist_free: not a whitelist of this context");
  HIPC(hipSetDevice(c->device));
  HIPC(hipStreamSynchronize(c->stream));   // (a kamd_bus_correct of the caller's may still read it)
  c->whitelists.erase(std::find(c->whitelists.begin(), c->whitelists.end(), wl));
  if (wl->slots) (void)hipFree(wl->slots);
  delete wl;
  return 0;
}

extern "C" int kamd_bus_correct(kamd_ctx* c, const kamd_bus_whitelist* wl, const kamd_bus_record* d_in, uint64_t n, kamd_bus_record* d_out, uint8_t* d_status,
                                uint64_t* n_out, kamd_bus_correct_stats* stats) {
  if (n_out) *n_out = 0;
  if (stats) memset(stats, 0, sizeof *stats);
  if (!c || !wl || !n_out) return kamd::fail(-1, "kamd_bus_correct: null argument");
  if (!owns(c, wl)) return kamd::fail(-1, "kamd_bus_correct: not a whitelist of this context");
  if (n >= 0xFFFFFFFFULL) return kamd::fail(-1, "kamd_bus_correct: a call takes fewer than 2^32 - 1 records");
  if (n == 0) return 0;
  if (!d_in || !d_out) return kamd::fail(-1, "kamd_bus_correct: null argument");
  if (misaligned(d_in) || misaligned(d_out)) return kamd::fail(-1, "kamd_bus_correct: the records must be 16-byte aligned");
  if (d_in < d_out + n && d_out < d_in + n) return kamd::fail(-1, "kamd_bus_correct: the output buffer must not overlap the input");
  if (int rc = events_ready(c)) return rc;
  const unsigned nb = grid_for(n, BLOCK);
  if (!d_status) { if (int rc = c->bcor_status.ensure(n, 0, c->stream)) return rc; }
  if (int rc = c->bcor_miss.ensure(n * sizeof(u32), 0, c->stream)) return rc;
  if (int rc = c->bcor_fix.ensure(n * sizeof(u64), 0, c->stream)) return rc;
  if (int rc = c->bcor_ctr.ensure(std::max(sizeof(WlCounters), sizeof(CorCounters)), 0, c->stream)) return rc;
  if (int rc = c->bus_blk.ensure((size_t)nb * sizeof(u32), 0, c->stream)) return rc;
  uint8_t* status = d_status ? d_status : c->bcor_status.as<uint8_t>();
  u32 *miss = c->bcor_miss.as<u32>(), *blk = c->bus_blk.as<u32>();
  u64* fix = c->bcor_fix.as<u64>();
  CorCounters* ctr = c->bcor_ctr.as<CorCounters>();
  const kamd::WlTable t{(const uint64_t*)wl->slots, (uint64_t)wl->n_buckets, wl->bc_len, wl->has_marker};
  // k_cor_neigh: a wavefront per miss, at most sixteen workgroups per compute unit and no more wavefronts than records
  const unsigned neigh_grid = (unsigned)std::min<u64>(grid_for(n, WAVES), (u64)std::max(c->n_cus, 1) * 16);
  const dim3 g(nb), th(BLOCK);
  HIPC(hipEventRecord(c->bus_ev[0], c->stream));
  HIPC(hipMemsetAsync(ctr, 0, sizeof *ctr, c->stream));
  hipLaunchKernelGGL(k_cor_exact, g, th, 0, c->stream, t, d_in, (u64)n, status, miss, ctr);
  HIPC(hipEventRecord(c->bcor_ev[0], c->stream));
  hipLaunchKernelGGL(k_cor_neigh, dim3(neigh_grid), th, 0, c->stream, t, d_in, (u64)n, (const u32*)miss, (const CorCounters*)ctr, status, fix);
  HIPC(hipEventRecord(c->bcor_ev[1], c->stream));
  hipLaunchKernelGGL(k_cor_count, g, th, 0, c->stream, (const uint8_t*)status, (u64)n, blk, ctr);
  hipLaunchKernelGGL(k_bus_scan, dim3(1), th, 0, c->stream, blk, (u64)nb, &ctr->n_out);
  hipLaunchKernelGGL(k_cor_scatter, g, th, 0, c->stream, d_in, (u64)n, (const uint8_t*)status, (const u64*)fix, (const u32*)blk, d_out);
  HIPC(hipGetLastError());
  HIPC(hipEventRecord(c->bus_ev[1], c->stream));
  CorCounters h{};
  HIPC(hipMemcpyAsync(&h, ctr, sizeof h, hipMemcpyDeviceToHost, c->stream));
  HIPC(hipStreamSynchronize(c->stream));   // the call's one synchronisation
  float ms = 0.f, neigh_ms = 0.f;
  HIPC(hipEventElapsedTime(&ms, c->bus_ev[0], c->bus_ev[1]));
  HIPC(hipEventElapsedTime(&neigh_ms, c->bcor_ev[0], c->bcor_ev[1]));
  *n_out = h.n_out;
  if (stats) {
    stats->n_in = n; stats->n_exact = h.n_status[0]; stats->n_corrected = h.n_status[1]; stats->n_ambiguous = h.n_status[2]; stats->n_uncorrectable = h.n_status[3];
    stats->n_out = h.n_out; stats->last_ms = ms; stats->neigh_ms = neigh_ms;
  }
  return 0;
}
