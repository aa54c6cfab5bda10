// kamd_em_stream.hip -- the EM's streamed form: its kernels (the passes themselves: kamd_em_stream.h), the one-time re-layout of the matrix,
// the launches of a round
#include "kamd_em_stream.h"

namespace {
// rows launch (first of the round: block 0 publishes the round's loop-control record, like k_em_rows)
template <int K, int PRE, bool WIN>
__global__ __launch_bounds__(PM_BLOCK) void k_pm_rows_pass(PmArgs A, int parity) {
  __shared__ double lds_sums[(PM_BLOCK / 64) * PM_LDS_SLOTS];
  const EmState prev = A.st[parity ^ 1];
  const u32 c = __builtin_amdgcn_readfirstlane(blockIdx.x * (PM_BLOCK / 64) + (threadIdx.x >> 6));
  PmWave<K> w;
  if (c < A.rows.n_chunks) pm_wave_load<K>(A.rows, c, w);
  const EmNow now = em_next_round(prev, A.n_iter, A.min_rounds, A.spec_hist != nullptr);
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    EmState r; r.iter = now.it; r.chcount = 0; r.final_round = now.fin; r.done = now.done; r.rounds = now.rounds; r.force_final = 0;
    r.pad[0] = r.pad[1] = 0;
    A.st[parity] = r;
    if (A.spec_hist && !prev.done && prev.iter >= 0) A.spec_hist[prev.iter] = prev.chcount;
  }
  if (now.done) return;
  const int odd = now.it & 1;
  if (c >= A.rows.n_chunks) return;
  const PmRowEmit em{A.cw, A.g};
  const double* a_cur = now.fin ? (odd ? A.ac1 : A.ac0) : (odd ? A.a1 : A.a0);
  pm_wave_pass<K, PRE, WIN>(A.rows, c, w, PmSrcGlobal{a_cur}, lds_sums + (threadIdx.x >> 6) * PM_LDS_SLOTS, em);
}
template <int K, int PRE, bool WIN>
__global__ __launch_bounds__(PM_BLOCK) void k_pm_cols_pass(PmArgs A, int parity) {
  __shared__ double lds_sums[(PM_BLOCK / 64) * PM_LDS_SLOTS];
  __shared__ int lds_ch;
  const EmState prev = A.st[parity ^ 1];
  const u32 c = __builtin_amdgcn_readfirstlane(blockIdx.x * (PM_BLOCK / 64) + (threadIdx.x >> 6));
  PmWave<K> w;
  if (c < A.cols.n_chunks) pm_wave_load<K>(A.cols, c, w);
  const EmNow now = em_next_round(prev, A.n_iter, A.min_rounds, A.spec_hist != nullptr);
  if (now.done) return;
  const int odd = now.it & 1;
  int ch = 0;
  const double* a_cur = now.fin ? (odd ? A.ac1 : A.ac0) : (odd ? A.a1 : A.a0);
  const PmColEmit em{odd ? A.alpha1 : A.alpha0, a_cur, A.single, A.eff, odd ? A.alpha0 : A.alpha1, odd ? A.a0 : A.a1, odd ? A.ac0 : A.ac1, &ch, now.fin};
  if (c < A.cols.n_chunks) pm_wave_pass<K, PRE, WIN>(A.cols, c, w, PmSrcGlobal{A.g}, lds_sums + (threadIdx.x >> 6) * PM_LDS_SLOTS, em);
  pm_count_changes(ch, &lds_ch, &A.st[parity]);
}
// fix-up launches (only enqueued when a direction has heavy crossing segments)
__global__ __launch_bounds__(PM_BLOCK) void k_pm_rows_fix(PmArgs A, int parity) {
  if (em_next_round(A.st[parity ^ 1], A.n_iter, A.min_rounds, A.spec_hist != nullptr).done) return;
  const PmRowEmit em{A.cw, A.g};
  pm_fix(A.rows, blockIdx.x * PM_BLOCK + threadIdx.x, em);
}
__global__ __launch_bounds__(PM_BLOCK) void k_pm_cols_fix(PmArgs A, int parity) {
  __shared__ int lds_ch;
  const EmNow now = em_next_round(A.st[parity ^ 1], A.n_iter, A.min_rounds, A.spec_hist != nullptr);
  if (now.done) return;
  const int odd = now.it & 1;
  int ch = 0;
  const double* a_cur = now.fin ? (odd ? A.ac1 : A.ac0) : (odd ? A.a1 : A.a0);
  const PmColEmit em{odd ? A.alpha1 : A.alpha0, a_cur, A.single, A.eff, odd ? A.alpha0 : A.alpha1, odd ? A.a0 : A.a1, odd ? A.ac0 : A.ac1, &ch, now.fin};
  pm_fix(A.cols, blockIdx.x * PM_BLOCK + threadIdx.x, em);
  pm_count_changes(ch, &lds_ch, &A.st[parity]);
}

// ---- one-time re-layout for the streamed form -------------------------------------------------------------------------
// Kept rows are renumbered by their smallest transcript id (a counting sort): rows of one gene become neighbours, and since
// the isoforms of a gene are neighbours in transcript space too, the 8-byte gathers of a wavefront fall into few cache
// lines (the passes are bound by the L2 request rate of uncoalesced gathers, not by bytes).
__global__ void k_pm_flags(const u64* __restrict__ ec_off, const u32* __restrict__ ec_ids, u64 n_ecs, const u32* __restrict__ col_cnt, u64 n_tr,
                           u32* hist, u32* mflag) {
  const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n_ecs) { const u64 a = ec_off[i]; if (ec_off[i + 1] - a >= 2) atomicAdd(&hist[ec_ids[a]], 1u); }   // sets are sorted: first = smallest
  if (i < n_tr) mflag[i] = col_cnt[i] ? 1u : 0u;
}
// The new number of a kept row: rows ordered by the bucket of their smallest transcript (4096 buckets over the transcripts: rows of one gene
// become neighbours, the gathers of a wavefront fall into few lines and a row block of the blocked form holds few genes' rows), rows of one
// bucket by a 48-bit hash of their CONTENT (the set of transcripts; equal sets do not occur).  The numbering -- and with it the order of every
// floating-point sum of the streamed and blocked forms -- is therefore a function of the matrix alone, whatever order kamd_ec_finalize's
// atomics emitted the classes in (until round 5 the place inside a group came from an atomic counter: abundances of an oversized component
// differed in the last bits from run to run).  A least-significant-digit radix sort of the rows by that 60-bit key, 12 bits per pass; a pass
// is a STABLE counting sort: one wavefront per tile of PM_RANK_TILE rows counts its rows per digit (k_pm_radix_hist), a scan over (digit, tile)
// gives every tile's first place in every digit, k_pm_radix_place walks the tile in order, 64 rows at a time.  Rows that are not kept (fewer
// than two transcripts) carry the largest key and end up behind the R kept ones.
constexpr int PM_RANK_BUCKETS = 4096, PM_RANK_TILE = 1024, PM_RANK_PASSES = 5;
__global__ void k_pm_rowkey(const u64* __restrict__ ec_off, const u32* __restrict__ ec_ids, u64 n_ecs, u64 n_tr, u64* key) {
  const u64 e = ((u64)blockIdx.x * blockDim.x + threadIdx.x) / 8;   // 8 lanes per row
  const int sub = threadIdx.x & 7;
  if (e >= n_ecs) return;
  const u64 a = ec_off[e], b = ec_off[e + 1];
  u64 h = 0;
  for (u64 j = a + sub; j < b; j += 8) h += kamd::mix64((u64)ec_ids[j] + 0x9e3779b97f4a7c15ULL);   // (a sum: the same for any order of the members)
  h += shfl_u64(h, lane_id() ^ 1); h += shfl_u64(h, lane_id() ^ 2); h += shfl_u64(h, lane_id() ^ 4);
  if (sub == 0) key[e] = b - a >= 2 ? (((u64)ec_ids[a] * PM_RANK_BUCKETS / n_tr) << 48) | (kamd::mix64(h) >> 16) : ~0ULL;
}
__device__ __forceinline__ u32 pm_radix_digit(u64 k, int pass) { return (u32)(k >> (12 * pass)) & (PM_RANK_BUCKETS - 1); }
// order_in == null: the identity (first pass)
__global__ __launch_bounds__(64) void k_pm_radix_hist(const u64* __restrict__ key, const u32* __restrict__ order_in, u64 n, int pass, u32 n_tiles, u32* hist) {
  __shared__ u32 s_cnt[PM_RANK_BUCKETS];
  const int lane = lane_id();
  for (int i = lane; i < PM_RANK_BUCKETS; i += 64) s_cnt[i] = 0u;
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  const u64 p0 = (u64)blockIdx.x * PM_RANK_TILE;
  for (u32 i = lane; i < (u32)PM_RANK_TILE; i += 64) {
    const u64 p = p0 + i;
    if (p < n) atomicAdd(&s_cnt[pm_radix_digit(key[order_in ? order_in[p] : p], pass)], 1u);
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  for (int i = lane; i < PM_RANK_BUCKETS; i += 64) hist[(u64)i * n_tiles + blockIdx.x] = s_cnt[i];
}
__global__ __launch_bounds__(64) void k_pm_radix_place(const u64* __restrict__ key, const u32* __restrict__ order_in, u64 n, int pass, u32 n_tiles,
                                                       const u64* __restrict__ first, u32* order_out) {
  __shared__ u32 s_cnt[PM_RANK_BUCKETS];   // rows of the tile placed so far, per digit
  const int lane = lane_id();
  for (int i = lane; i < PM_RANK_BUCKETS; i += 64) s_cnt[i] = 0u;
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  const u64 p0 = (u64)blockIdx.x * PM_RANK_TILE;
  for (u32 i0 = 0; i0 < (u32)PM_RANK_TILE; i0 += 64) {
    const u64 p = p0 + i0 + lane;
    const bool in = p < n;
    const u32 e = in ? (order_in ? order_in[p] : (u32)p) : 0u;
    const u32 dg = in ? pm_radix_digit(key[e], pass) : 0xFFFFFFFFu;
    // the lanes of one digit, in lane order: one leader per distinct digit and trip
    u64 todo = __ballot(in);
    u32 before = 0, same_total = 0;
    while (todo) {
      const int leader = __ffsll((long long)todo) - 1;
      const u32 ld = (u32)__shfl((int)dg, leader, 64);
      const u64 same = __ballot(dg == ld);
      if (dg == ld) { before = (u32)__popcll(same & ((1ULL << lane) - 1ULL)); same_total = (u32)__popcll(same); }
      todo &= ~same;
    }
    if (in) order_out[first[(u64)dg * n_tiles + blockIdx.x] + s_cnt[dg] + before] = e;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    if (in && before == 0) s_cnt[dg] += same_total;   // (the first lane of every digit)
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  }
}
// the sorted order -> the kept rows' new numbers and lengths (the R kept rows come first)
__global__ void k_pm_rank_emit(const u64* __restrict__ ec_off, const u32* __restrict__ order, u64 R, u64* rpos, u32* len_sorted) {
  const u64 r = (u64)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= R) return;
  const u32 e = order[r];
  rpos[e] = r;
  len_sorted[r] = (u32)(ec_off[e + 1] - ec_off[e]);
}
// kept row e -> entries of the row stream, its count word and offset; 8 lanes per row
__global__ void k_pm_rows(const u64* __restrict__ ec_off, const u32* __restrict__ ec_ids, const u32* __restrict__ counts,
                          const u32* __restrict__ wcounts, u64 n_ecs, const u64* __restrict__ rpos, const u64* __restrict__ roff,
                          const u64* __restrict__ mpos, u32* stream, u64* cw) {
  const u64 e = ((u64)blockIdx.x * blockDim.x + threadIdx.x) / 8;
  const int sub = threadIdx.x & 7;
  if (e >= n_ecs) return;
  const u64 a = ec_off[e], b = ec_off[e + 1];
  if (b - a < 2) return;
  const u64 r = rpos[e], base = roff[r];
  for (u64 j = a + sub; j < b; j += 8) stream[base + (j - a)] = (u32)mpos[ec_ids[j]] | (j + 1 == b ? PM_END : 0u);
  if (sub == 0) cw[r] = (u64)counts[e] | ((u64)wcounts[e] << 32);
}
__global__ void k_pm_cols(const u64* __restrict__ ec_off, const u32* __restrict__ ec_ids, u64 n_ecs, const u64* __restrict__ rpos,
                          const u64* __restrict__ col_off, u32* col_fill, u32* stream) {
  const u64 e = ((u64)blockIdx.x * blockDim.x + threadIdx.x) / 8;
  const int sub = threadIdx.x & 7;
  if (e >= n_ecs) return;
  const u64 a = ec_off[e], b = ec_off[e + 1];
  if (b - a < 2) return;
  const u32 r = (u32)rpos[e];
  for (u64 j = a + sub; j < b; j += 8) {
    const u32 t = ec_ids[j];
    const u64 p = col_off[t] + atomicAdd(&col_fill[t], 1u);
    stream[p] = r | (p + 1 == col_off[t + 1] ? PM_END : 0u);
  }
}
__global__ void k_pm_fill(u32* p, u64 a, u64 b, u32 v) {
  const u64 i = a + (u64)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < b) p[i] = v;
}
// m-space vectors; alpha_ = 1/T for every transcript (:38)
__global__ void k_pm_minit(u64 n_tr, const u32* __restrict__ mflag, const u64* __restrict__ mpos, const u64* __restrict__ col_off,
                           const double* __restrict__ single, const double* __restrict__ eff, u64 M, u64* coff, double* single_m,
                           double* eff_m, double* alpha0, double* alpha1, double* a0, double* a1, double* ac0, double* ac1) {
  const u64 t = (u64)blockIdx.x * blockDim.x + threadIdx.x;
  if (t == 0) { if (coff) coff[M] = col_off[n_tr]; alpha0[M] = alpha1[M] = a0[M] = a1[M] = ac0[M] = ac1[M] = 0.0; }
  if (t >= n_tr || !mflag[t]) return;
  const u64 m = mpos[t];
  if (coff) coff[m] = col_off[t];   // (null: a cached plan gets new counts and effective lengths, its layout stays)
  single_m[m] = single[t]; eff_m[m] = eff[t];
  const double al = 1.0 / (double)n_tr;
  alpha0[m] = al; a0[m] = al / eff[t]; alpha1[m] = 0.0; a1[m] = 0.0;
  ac0[m] = al < 1e-7 / 10.0 ? 0.0 : al / eff[t]; ac1[m] = 0.0;
}
// per chunk: the segment its first entry belongs to (binary search in the segment offsets) and how it is completed
__global__ void k_pm_chunks(const u64* __restrict__ off, u64 n_seg, u64 nz, u32 chunk, u32 n_chunks, u32* seg_base, u32* head,
                            u32* fix_first, u32* n_fix, u32* max_ends, int no_long) {
  const u32 c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= n_chunks) return;
  const u64 c0 = (u64)c * chunk, c1 = c0 + chunk;
  u64 lo = 0, hi = n_seg;  // largest s in [0, n_seg) with off[s] <= c0 (off[0] = 0, offsets strictly increase)
  while (hi - lo > 1) { const u64 mid = (lo + hi) / 2; if (off[mid] <= c0) lo = mid; else hi = mid; }
  const u64 hs = off[lo], se = off[lo + 1];
  const u64 hl = c0 - hs;  // entries of the segment before the chunk
  // (a long head is only re-read by the chunk the segment ENDS in: a chunk wholly inside the segment would gather its hl preceding entries every
  // round and throw the sum away -- O(L^2 / chunk) wasted gathers per long segment; such chunks are marked heavy and need nothing but their own sum)
  const bool is_long = hl > 64ULL * PM_HEAD && hl <= (u64)PM_LOOP_MAX && !no_long && se <= c1;
  const bool is_heavy = hl > 64ULL * PM_HEAD && !is_long;
  seg_base[c] = (u32)lo;
  head[c] = hl == 0 ? 0u : (is_heavy ? PM_HEAVY : (is_long ? (PM_LONG | (u32)hl) : (u32)hl));
  const bool fix = is_heavy && se <= c1;
  fix_first[c] = fix ? (u32)(hs / chunk) : PM_NONE;
  if (fix) atomicAdd(n_fix, 1u);
  const u64 ce = c1 < nz ? c1 : nz;   // segment ends inside the chunk: segments lo .. l2 - 1, l2 = largest s in [0, n_seg] with off[s] <= ce
  u64 l2 = lo; hi = n_seg + 1;
  while (hi - l2 > 1) { const u64 mid = (l2 + hi) / 2; if (off[mid] <= ce) l2 = mid; else hi = mid; }
  if (l2 - lo > (u64)PM_LDS_SLOTS) atomicMax(max_ends, (u32)(l2 - lo));
}
// per lane of every chunk: PmSide::lane_word; one wavefront per chunk, any K
__global__ __launch_bounds__(PM_BLOCK) void k_pm_lanes(const u32* __restrict__ stream, u32 k, u32 n_chunks, u32* lane_word) {
  const u32 c = blockIdx.x * (PM_BLOCK / 64) + (threadIdx.x >> 6);
  if (c >= n_chunks) return;
  const int lane = lane_id();
  const u32* p = stream + (u64)c * (64 * k) + (u64)lane * k;
  u32 ne = 0;
  for (u32 i = 0; i < k; i++) ne += p[i] >> 31;
  const u32 incl = pm_scan_incl(ne);
  const u64 heads = __ballot(ne > 0);
  const u64 below = heads & ((2ULL << lane) - 1ULL);
  const u32 reach = below ? (u32)(lane - (63 - __clzll((long long)below))) : (u32)(lane + 1);
  lane_word[(u64)c * 64 + lane] = (incl - ne) | (ne << 12) | (reach << 18);
}
// ---- streamed EM: re-layout of the matrix (once per run) and the per-round launches -------------------------------------
constexpr int PM_KS[] = {8, 12, 16, 20, 24, 28, 32};
template <int K>
void pm_launch_round(const PmPlan& P, hipStream_t s, int parity) {
  const unsigned grid = grid_for(P.n_chunks, PM_BLOCK / 64);
  constexpr int PRE_R = (K + 5) / 6 < 2 ? 2 : (K + 5) / 6;   // 64 * PRE >= ~chunk / 6 row ends
  constexpr int PRE_C = K / 16 + 1;                           // 64 * PRE >= ~chunk / 16 column ends
  if (P.windowed) hipLaunchKernelGGL((k_pm_rows_pass<K, PRE_R, true>), dim3(grid), dim3(PM_BLOCK), 0, s, P.args, parity);
  else hipLaunchKernelGGL((k_pm_rows_pass<K, PRE_R, false>), dim3(grid), dim3(PM_BLOCK), 0, s, P.args, parity);
  if (P.n_fix[0]) hipLaunchKernelGGL(k_pm_rows_fix, dim3(grid_for(P.n_chunks, PM_BLOCK)), dim3(PM_BLOCK), 0, s, P.args, parity);
  if (P.windowed) hipLaunchKernelGGL((k_pm_cols_pass<K, PRE_C, true>), dim3(grid), dim3(PM_BLOCK), 0, s, P.args, parity);
  else hipLaunchKernelGGL((k_pm_cols_pass<K, PRE_C, false>), dim3(grid), dim3(PM_BLOCK), 0, s, P.args, parity);
  if (P.n_fix[1]) hipLaunchKernelGGL(k_pm_cols_fix, dim3(grid_for(P.n_chunks, PM_BLOCK)), dim3(PM_BLOCK), 0, s, P.args, parity);
}
}  // namespace
namespace kamdi {
void pm_enqueue_round(const PmPlan& P, hipStream_t s, int parity) {
  switch (P.k) {
    case 8: pm_launch_round<8>(P, s, parity); break;
    case 12: pm_launch_round<12>(P, s, parity); break;
    case 16: pm_launch_round<16>(P, s, parity); break;
    case 20: pm_launch_round<20>(P, s, parity); break;
    case 24: pm_launch_round<24>(P, s, parity); break;
    case 28: pm_launch_round<28>(P, s, parity); break;
    default: pm_launch_round<32>(P, s, parity); break;
  }
}

// returns 0 = plan built (the rounds can be enqueued with pm_enqueue_round), 1 = not applicable (the caller uses the CSR
// form), < 0 = error.  Needs col_cnt / em_coloff / em_single / em_eff of the caller (k_em_prepare + scan) and a zeroed col_fill.
int em_streamed_setup(kamd_ctx* c, const u64* ec_off, const u32* ec_ids, const u32* counts, const u32* wcounts, u64 n_ecs, u64 T,
                      const u32* col_cnt, u32* col_fill, PmPlan* P, DBuf* arena_a, DBuf* arena_b) {
  if (n_ecs == 0) return 1;
  DBuf& ar_a = arena_a ? *arena_a : c->pm_a;   // (the hybrid keeps the streamed plan of the oversized components in arenas of its own: pm_a / pm_b
  DBuf& ar_b = arena_b ? *arena_b : c->pm_b;   //  hold the LDS form's plan and vectors at the same time)
  if (c->n_cus == 0) {
    int v = 0;
    HIPC(hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, c->device));
    c->n_cus = v > 0 ? v : 256;
  }
  // stage 1: which rows / transcripts are kept, and their new numbers (rows: counting sort by smallest transcript)
  Carver s1;
  const size_t o_hist = s1.take((T + 1) * 4), o_fill = s1.take((T + 1) * 4), o_mflag = s1.take(T * 4);
  const size_t o_start = s1.take((T + 2) * 8), o_rpos = s1.take((n_ecs + 1) * 8), o_mpos = s1.take((T + 1) * 8);
  const size_t o_len = s1.take((n_ecs + 1) * 4), o_roff = s1.take((n_ecs + 2) * 8);
  if (int rc = ar_a.ensure(s1.off, 0, c->stream)) return rc;
  char* b1 = (char*)ar_a.p;
  u32* hist = (u32*)(b1 + o_hist); u32* mflag = (u32*)(b1 + o_mflag);
  u64* start = (u64*)(b1 + o_start); u64* rpos = (u64*)(b1 + o_rpos); u64* mpos = (u64*)(b1 + o_mpos);
  u32* len_sorted = (u32*)(b1 + o_len); u64* roff = (u64*)(b1 + o_roff);
  (void)o_fill;
  HIPC(hipMemsetAsync(hist, 0, (o_mflag - o_hist), c->stream));
  hipLaunchKernelGGL(k_pm_flags, dim3(grid_for(std::max(n_ecs, T), BLOCK)), dim3(BLOCK), 0, c->stream, ec_off, ec_ids, n_ecs, col_cnt, T, hist,
                     mflag);
  if (int rc = exclusive_scan(c, hist, T, start, start + T)) return rc;
  if (int rc = exclusive_scan(c, mflag, T, mpos, mpos + T)) return rc;
  u64 R = 0, NZ = 0, M = 0;
  HIPC(hipMemcpyAsync(&R, start + T, 8, hipMemcpyDeviceToHost, c->stream));
  HIPC(hipMemcpyAsync(&M, mpos + T, 8, hipMemcpyDeviceToHost, c->stream));
  HIPC(hipMemcpyAsync(&NZ, c->em_coloff.as<u64>() + T, 8, hipMemcpyDeviceToHost, c->stream));   // non-zeros of the kept rows
  HIPC(hipStreamSynchronize(c->stream));
  if (NZ == 0 || R == 0 || M == 0 || R >= 0x7FFFFFF0ULL || M >= 0x7FFFFFF0ULL || NZ >= (1ULL << 40)) return 1;
  {
    if (n_ecs >= 0xFFFFFFF0ULL) return 1;
    const u32 n_tiles = (u32)((n_ecs + PM_RANK_TILE - 1) / PM_RANK_TILE);
    const u64 n_cells = (u64)PM_RANK_BUCKETS * n_tiles;
    Carver rv;
    const size_t o_key = rv.take(n_ecs * 8), o_oa = rv.take(n_ecs * 4), o_ob = rv.take(n_ecs * 4), o_h = rv.take(n_cells * 4), o_f = rv.take((n_cells + 2) * 8);
    if (int rc = c->pm_rank.ensure(rv.off, 0, c->stream)) return rc;
    char* rb = (char*)c->pm_rank.p;
    u64* key = (u64*)(rb + o_key); u32* ord[2] = {(u32*)(rb + o_oa), (u32*)(rb + o_ob)}; u32* rhist = (u32*)(rb + o_h); u64* rfirst = (u64*)(rb + o_f);
    hipLaunchKernelGGL(k_pm_rowkey, dim3(grid_for(n_ecs * 8, BLOCK)), dim3(BLOCK), 0, c->stream, ec_off, ec_ids, n_ecs, T, key);
    const u32* in = nullptr;
    for (int pass = 0; pass < PM_RANK_PASSES; pass++) {
      u32* out = ord[pass & 1];
      hipLaunchKernelGGL(k_pm_radix_hist, dim3(n_tiles), dim3(64), 0, c->stream, (const u64*)key, in, n_ecs, pass, n_tiles, rhist);
      if (int rc = exclusive_scan(c, rhist, n_cells, rfirst, rfirst + n_cells)) return rc;
      hipLaunchKernelGGL(k_pm_radix_place, dim3(n_tiles), dim3(64), 0, c->stream, (const u64*)key, in, n_ecs, pass, n_tiles, (const u64*)rfirst, out);
      in = out;
    }
    hipLaunchKernelGGL(k_pm_rank_emit, dim3(grid_for(R, BLOCK)), dim3(BLOCK), 0, c->stream, ec_off, in, R, rpos, len_sorted);
    HIPC(hipGetLastError());
  }
  if (int rc = exclusive_scan(c, len_sorted, R, roff, roff + R)) return rc;   // roff[R] = NZ
  // entries per lane: the smallest K whose chunks fit the chip in one go at 12 wavefronts per CU (measured on config #3:
  // 28.0 us per round at K = 24 / 3038 chunks against 32.7 at K = 20 / 3646 and 32.5 at K = 16 / 4557, same box)
  int K = PM_KS[sizeof(PM_KS) / sizeof(PM_KS[0]) - 1];
  bool k_forced = false;
  if (c->tune.em_entries_per_lane > 0) { for (int k : PM_KS) if (k == c->tune.em_entries_per_lane) { K = k; k_forced = true; } }
  if (!k_forced) for (int k : PM_KS) if ((NZ + 64ULL * k - 1) / (64ULL * k) <= (u64)c->n_cus * 12) { K = k; break; }
  const u32 chunk = 64u * (u32)K;
  const u64 n_chunks64 = (NZ + chunk - 1) / chunk;
  if (n_chunks64 >= 0x7FFFFFF0ULL) return 1;
  const u32 n_chunks = (u32)n_chunks64;
  const u64 nzpad = (u64)n_chunks * chunk;
  // stage 2
  Carver s2;
  const size_t front = 64 * PM_HEAD * 4;   // the passes read up to 64 * PM_HEAD entries before a chunk, also before chunk 0
  const size_t o_rs = s2.take(front + nzpad * 4), o_cs = s2.take(front + nzpad * 4);
  size_t o_meta[2][5];
  size_t o_lane[2];
  for (int s = 0; s < 2; s++) {
    for (int j = 0; j < 3; j++) o_meta[s][j] = s2.take((size_t)n_chunks * 4);
    for (int j = 3; j < 5; j++) o_meta[s][j] = s2.take((size_t)n_chunks * 8);
    o_lane[s] = s2.take((size_t)n_chunks * 64 * 4);
  }
  const size_t o_cw = s2.take(R * 8), o_coff = s2.take((M + 1) * 8), o_g = s2.take((R + 1) * 8);
  size_t o_vec[6];
  for (int j = 0; j < 6; j++) o_vec[j] = s2.take((M + 1) * 8);
  const size_t o_single = s2.take(M * 8), o_eff = s2.take(M * 8), o_nfix = s2.take(64);
  if (int rc = ar_b.ensure(s2.off, 0, c->stream)) return rc;
  char* b2 = (char*)ar_b.p;
  u32* rs = (u32*)(b2 + o_rs + front); u32* cs = (u32*)(b2 + o_cs + front);
  HIPC(hipMemsetAsync(b2 + o_rs, 0, front, c->stream));
  HIPC(hipMemsetAsync(b2 + o_cs, 0, front, c->stream));
  u64* cw = (u64*)(b2 + o_cw); u64* coff = (u64*)(b2 + o_coff);
  double* g = (double*)(b2 + o_g);
  double* vec[6]; for (int j = 0; j < 6; j++) vec[j] = (double*)(b2 + o_vec[j]);
  double* single_m = (double*)(b2 + o_single); double* eff_m = (double*)(b2 + o_eff);
  HIPC(hipMemsetAsync(b2 + o_nfix, 0, 64, c->stream));
  HIPC(hipMemsetAsync(g + R, 0, 8, c->stream));
  const u64* col_off = c->em_coloff.as<u64>();
  hipLaunchKernelGGL(k_pm_rows, dim3(grid_for(n_ecs * 8, BLOCK)), dim3(BLOCK), 0, c->stream, ec_off, ec_ids, counts, wcounts, n_ecs, rpos, roff,
                     mpos, rs, cw);
  hipLaunchKernelGGL(k_pm_cols, dim3(grid_for(n_ecs * 8, BLOCK)), dim3(BLOCK), 0, c->stream, ec_off, ec_ids, n_ecs, rpos, col_off, col_fill, cs);
  if (nzpad > NZ) {
    hipLaunchKernelGGL(k_pm_fill, dim3(grid_for(nzpad - NZ, BLOCK)), dim3(BLOCK), 0, c->stream, rs, NZ, nzpad, (u32)M);
    hipLaunchKernelGGL(k_pm_fill, dim3(grid_for(nzpad - NZ, BLOCK)), dim3(BLOCK), 0, c->stream, cs, NZ, nzpad, (u32)R);
  }
  hipLaunchKernelGGL(k_pm_minit, dim3(grid_for(T, BLOCK)), dim3(BLOCK), 0, c->stream, T, mflag, mpos, col_off, c->em_single.as<double>(),
                     c->em_eff.as<double>(), M, coff, single_m, eff_m, vec[0], vec[1], vec[2], vec[3], vec[4], vec[5]);
  PmSide sides[2];
  for (int s = 0; s < 2; s++) {
    PmSide& d = sides[s];
    d.stream = s == 0 ? rs : cs;
    u32* sb = (u32*)(b2 + o_meta[s][0]); u32* hd = (u32*)(b2 + o_meta[s][1]); u32* ff = (u32*)(b2 + o_meta[s][2]);
    d.seg_base = sb; d.head = hd; d.fix_first = ff;
    d.lp = (double*)(b2 + o_meta[s][3]); d.rp = (double*)(b2 + o_meta[s][4]);
    d.n_chunks = n_chunks;
    u32* lw = (u32*)(b2 + o_lane[s]);
    d.lane_word = lw;
    hipLaunchKernelGGL(k_pm_lanes, dim3(grid_for(n_chunks, PM_BLOCK / 64)), dim3(PM_BLOCK), 0, c->stream, d.stream, chunk / 64, n_chunks, lw);
    hipLaunchKernelGGL(k_pm_chunks, dim3(grid_for(n_chunks, BLOCK)), dim3(BLOCK), 0, c->stream, s == 0 ? roff : coff, s == 0 ? R : M, NZ, chunk,
                       n_chunks, sb, hd, ff, (u32*)(b2 + o_nfix) + s, (u32*)(b2 + o_nfix) + 2, getenv("KAMD_EM_NO_LONG_HEADS") ? 1 : 0);
  }
  HIPC(hipGetLastError());
  PmArgs& A = P->args;
  A.rows = sides[0]; A.cols = sides[1];
  A.cw = cw; A.g = g;
  A.alpha0 = vec[0]; A.alpha1 = vec[1]; A.a0 = vec[2]; A.a1 = vec[3]; A.ac0 = vec[4]; A.ac1 = vec[5];
  A.single = single_m; A.eff = eff_m;
  A.R = (u32)R; A.M = (u32)M;
  A.st = (EmState*)c->em_state.p;
  u32 plan_words[3] = {0, 0, 0};   // heavy crossings per direction, largest number of segment ends in a chunk (if above the LDS slots)
  HIPC(hipMemcpyAsync(plan_words, b2 + o_nfix, sizeof plan_words, hipMemcpyDeviceToHost, c->stream));
  HIPC(hipStreamSynchronize(c->stream));
  P->n_fix[0] = plan_words[0]; P->n_fix[1] = plan_words[1];
  P->windowed = plan_words[2] > (u32)PM_LDS_SLOTS;
  if (c->tune.em_windowed == 1) P->windowed = true;
  P->k = K; P->n_chunks = n_chunks; P->mflag = mflag; P->mpos = mpos; P->rpos = rpos;
  P->roff = roff; P->coff = coff; P->rs = rs; P->cs = cs; P->nzpad = nzpad;
  c->last_em_nnz_multi = NZ; c->last_em_nseg = n_chunks; c->last_em_necs = n_ecs; c->last_em_k = K;
  c->last_em_grid = grid_for(n_chunks, PM_BLOCK / 64);
  return 0;
}
void pm_refresh_enqueue(kamd_ctx* c, const PmPlan& P, u64 T) {
  const PmArgs& A = P.args;
  hipLaunchKernelGGL(k_pm_minit, dim3(grid_for(T, BLOCK)), dim3(BLOCK), 0, c->stream, T, P.mflag, P.mpos, (const u64*)nullptr, (const double*)c->em_single.as<double>(),
                     (const double*)c->em_eff.as<double>(), (u64)A.M, (u64*)nullptr, const_cast<double*>(A.single), const_cast<double*>(A.eff), A.alpha0, A.alpha1, A.a0, A.a1, A.ac0, A.ac1);
}
}  // namespace kamdi
