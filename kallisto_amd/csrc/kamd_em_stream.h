// kamd_em_stream.h -- device code of the streamed EM passes: what the streamed form's kernels (k_pm_*, kamd_em_stream.hip) and the hybrid's
// kernels for the oversized components (k_gi_*, k_gb_*, kamd_em.hip) both instantiate; k_em_sell (kamd_em.hip) takes the wavefront scans.
#pragma once
#include "kamd_em_int.h"

namespace {
// ------------------------------------------------------------------------------------------------------------------
// Kernel B, streamed form: two launches per round (rows, columns) over a re-laid-out matrix.  At the sizes of a
// transcriptome (a few 1e6 non-zeros) a round is bound by dependent-load latency and launch count, not by bytes: the CSR
// form above chases row offsets -> ids -> a[] (three dependent latencies per kernel, three kernels).  Re-layout, once per run:
//   * only rows with >= 2 transcripts and only transcripts that occur in such a row are kept ("m-space", compact ids);
//     singleton rows are the constant single[] term of their transcript
//   * both directions of the matrix are FLAGGED STREAMS: entry = index | PM_END on the last entry of a row (column).
//     No offset arrays are read in the loop.  A wavefront owns one chunk of 64 x K consecutive entries (each lane K
//     consecutive ones: K/4 16-byte loads, then K independent 8-byte gathers -- two dependent memory latencies per launch),
//     reduces them with a lane-local pass + ONE segmented wavefront scan, stages the segment sums in LDS and finishes them
//     lane-parallel (coalesced constants and stores, no divergent divisions)
//   * a segment that crosses into a chunk from the left is re-read by that chunk if the part outside is short (<= 256
//     entries, loads issued together with the chunk's own), else completed by a small fix-up launch from the chunks'
//     left/right partial sums in chunk order (deterministic summation, no floating-point atomics); that launch only exists
//     when such segments do
// A persistent single-launch form with grid barriers was built and measured first (scratch/em_persistent_kernel_attempt):
// one grid barrier costs 4.9-6.3 us on 256 CUs (kamd_debug_grid_barrier), a kernel boundary ~1.7 us, so launches win.
// ------------------------------------------------------------------------------------------------------------------
// Wavefront scans on the DPP data path (row_shr within the rows of 16 lanes, then row_bcast:15 / row_bcast:31 across
// rows): six VALU steps instead of six LDS round trips (__shfl_up is ds_bpermute_b32, ~100+ cycles each, and the steps of
// a scan depend on each other).
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ u32 pm_dpp(u32 v) { return (u32)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, ROW_MASK, 0xF, true); }
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ double pm_dpp(double v) {
  const u32 lo = pm_dpp<CTRL, ROW_MASK>((u32)__double2loint(v)), hi = pm_dpp<CTRL, ROW_MASK>((u32)__double2hiint(v));
  return __hiloint2double((int)hi, (int)lo);
}
__device__ __forceinline__ u32 pm_scan_incl(u32 x) {   // inclusive prefix sum over the 64 lanes
  x += pm_dpp<0x111, 0xF>(x); x += pm_dpp<0x112, 0xF>(x); x += pm_dpp<0x114, 0xF>(x); x += pm_dpp<0x118, 0xF>(x);
  x += pm_dpp<0x142, 0xA>(x);   // row_bcast:15 into rows 1 and 3
  x += pm_dpp<0x143, 0xC>(x);   // row_bcast:31 into rows 2 and 3
  return x;
}
// segmented inclusive sum: lane l gets the sum over lanes (l - reach, l] where reach = distance to the nearest segment
// start at or below l (0: the lane starts a segment itself; l + 1: none below)
__device__ __forceinline__ double pm_scan_seg(double y, int reach, int lane) {
  const int r = lane & 15;   // position inside the row
  { const double t = pm_dpp<0x111, 0xF>(y); if (reach >= 1 && r >= 1) y += t; }
  { const double t = pm_dpp<0x112, 0xF>(y); if (reach >= 2 && r >= 2) y += t; }
  { const double t = pm_dpp<0x114, 0xF>(y); if (reach >= 4 && r >= 4) y += t; }
  { const double t = pm_dpp<0x118, 0xF>(y); if (reach >= 8 && r >= 8) y += t; }
  // rows 1 and 3 take the total of the row before them if their run reaches back past the row's first lane
  { const double t = pm_dpp<0x142, 0xA>(y); if ((lane & 16) && reach > r) y += t; }
  // rows 2 and 3 take lane 31's value if their run reaches back past lane 32
  { const double t = pm_dpp<0x143, 0xC>(y); if (lane >= 32 && reach > lane - 32) y += t; }
  return y;
}
__device__ __forceinline__ double pm_wave_sum(double x) {   // sum over the 64 lanes, in every lane
  x += pm_dpp<0x111, 0xF>(x); x += pm_dpp<0x112, 0xF>(x); x += pm_dpp<0x114, 0xF>(x); x += pm_dpp<0x118, 0xF>(x);
  x += pm_dpp<0x142, 0xA>(x); x += pm_dpp<0x143, 0xC>(x);
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(x), 63), __builtin_amdgcn_readlane(__double2loint(x), 63));
}
// what is done with a finished segment sum: load() fetches the segment's constants (issued before the sums are known,
// coalesced: consecutive lanes finish consecutive segments), finish() consumes them with the sum
struct PmRowEmit {   // g_e = count_e / S_e; rows the reference skips get 0: count 0 (:133-135), denom below denorm_min (:156-158)
  const u64* cw; double* g;
  using Ctx = u64;
  __device__ __forceinline__ Ctx load(u32 r) const { return cw[r]; }
  __device__ __forceinline__ void finish(u32 r, const Ctx& w, double S) const {
    const u32 cnt = (u32)w, wc = (u32)(w >> 32);
    g[r] = (cnt == 0 || (double)wc * S < 4.9406564584124654e-324) ? 0.0 : (double)cnt / S;
  }
};
struct PmColEmit {   // next_t = single_t + a_t * sum_e g_e and the convergence test of :176-199
  const double* alpha_cur; const double* a_cur; const double* single; const double* eff;
  double* alpha_nx; double* a_nx; double* ac_nx; int* ch; int clamp;   // a_cur is the clamped copy in the final round
  struct Ctx { double al, at, sg, ef; };
  __device__ __forceinline__ Ctx load(u32 m) const { return Ctx{alpha_cur[m], a_cur[m], single[m], eff[m]}; }
  __device__ __forceinline__ void finish(u32 m, const Ctx& x, double acc) const {
    const double al = (clamp && x.al < 1e-7 / 10.0) ? 0.0 : x.al;
    const double nx = x.sg + x.at * acc;
    if (nx > 1e-2 && (fabs(nx - al) / nx) > 1e-2) ++*ch;
    const double an = nx / x.ef;
    alpha_nx[m] = nx;
    a_nx[m] = an;
    ac_nx[m] = nx < 1e-7 / 10.0 ? 0.0 : an;
  }
};

// one wavefront, one chunk: value of entry j = src[index_j]; every segment that ends in the chunk is finished here unless it
// crossed in from far to the left (PM_HEAVY: pm_fix)
// (in two steps so that the kernels can issue the chunk's loads BEFORE they use the round's loop-control record: both are
// first-touch reads of a cold L2, ~2 us each, overlapped instead of chained)
template <int K>
struct PmWave { u32 id[K]; u32 hraw[PM_HEAD]; u32 sb, hd, lw; };
template <int K>
__device__ __forceinline__ void pm_wave_load(const PmSide& s, u32 c, PmWave<K>& w) {
  const uint4* p = reinterpret_cast<const uint4*>(s.stream + (u64)c * (64 * K) + lane_id() * K);
#pragma unroll
  for (int q = 0; q < K / 4; q++) { const uint4 x = p[q]; w.id[4 * q] = x.x; w.id[4 * q + 1] = x.y; w.id[4 * q + 2] = x.z; w.id[4 * q + 3] = x.w; }
  // the 64 * PM_HEAD entries before the chunk (the stream has that much padding in front): which of them belong to the
  // segment that crosses into the chunk is known once head[c] is here, their addresses do not depend on it
  const u32* hb = s.stream + (u64)c * (64 * K) + lane_id();
#pragma unroll
  for (int i = 0; i < PM_HEAD; i++) w.hraw[i] = *(hb - 64 * (i + 1));
  w.sb = s.seg_base[c];
  w.hd = s.head[c];
  w.lw = s.lane_word[(u64)c * 64 + lane_id()];
}
// where the value of an entry comes from (the blocked passes of an oversized component read a block of the vector out of LDS instead)
struct PmSrcGlobal {
  const double* __restrict__ p;
  __device__ __forceinline__ double operator()(u32 id) const { return p[id & ~PM_END]; }
};
template <int K, int PRE, bool WIN, class Emit, class Src>
__device__ __forceinline__ void pm_wave_pass(const PmSide& s, u32 c, PmWave<K>& w, const Src& src, double* lds, const Emit& em) {
  const int lane = lane_id();
  u32 (&id)[K] = w.id;
  const u32 sb = w.sb;
  const u32 hd = w.hd;
  const bool heavy = (hd & PM_HEAVY) != 0;
  const bool longhead = !heavy && (hd & PM_LONG) != 0;
  const u32 hlen = heavy ? 0u : (hd & ~PM_LONG);
  // lane l holds the entries 64 * (i + 1) - l before the chunk
  // A LONG head (a row / column of hundreds to thousands of entries that crosses into the chunk: repeat-family and poly-A classes, hub
  // transcripts) is re-read in a loop, 64 entries per trip -- the trips are independent, so the chunk pays one more latency and a few
  // dozen issue slots, where the fix-up launch it replaces cost a kernel boundary and a launch per direction and round (4.7 + 4.6 us
  // each on the stress workload: 4 launches per round -> 2).  The entries are summed lane-strided, then across the lanes: a fixed order.
  auto head_sum = [&](void) -> double {
    double hv[PM_HEAD];
#pragma unroll
    for (int i = 0; i < PM_HEAD; i++) hv[i] = src(w.hraw[i]);
    double hs = 0.0;
#pragma unroll
    for (int i = 0; i < PM_HEAD; i++) hs += (u32)(64 * (i + 1) - lane) <= hlen ? hv[i] : 0.0;
    if (longhead) {
      const u32* before = s.stream + (u64)c * (64 * K);   // entry i of the head (counted backwards from the chunk) at before[-1 - i]
      u32 i = 64 * PM_HEAD + (u32)lane;
      for (; i + 192 < hlen; i += 256) {   // four independent gathers per trip
        const u32 i0 = before[-1 - (long)i], i1 = before[-1 - (long)(i + 64)], i2 = before[-1 - (long)(i + 128)], i3 = before[-1 - (long)(i + 192)];
        const double v0 = src(i0), v1 = src(i1), v2 = src(i2), v3 = src(i3);
        hs += v0; hs += v1; hs += v2; hs += v3;
      }
      for (; i < hlen; i += 64) hs += src(before[-1 - (long)i]);
    }
    return hs;
  };
  const u32 skip = heavy ? 1u : 0u;   // a heavy crossing segment's end is finished by pm_fix
  // (the END flag stays in id[k]: its sign is the "this entry ends a segment" test of the loops below)
  if constexpr (!WIN) {
    const u32 ebase = w.lw & 0xFFFu, ne = (w.lw >> 12) & 0x3Fu;
    const int reach = (int)(w.lw >> 18);
    const u32 n_ends = (u32)__builtin_amdgcn_readlane((int)(ebase + ne), 63);
    // every segment end of the chunk has its own LDS slot (all real chunks): no window tests, and the lane's first end is
    // staged like the others and completed in place once the carry is known -- 6 instructions per entry instead of ~25
    double v[K];
#pragma unroll
    for (int k = 0; k < K; k++) v[k] = src(id[k]);
    double hsum = head_sum();
    typename Emit::Ctx pre[PRE];
#pragma unroll
    for (int i = 0; i < PRE; i++) { const u32 j = skip + lane + 64 * i; if (j < n_ends) pre[i] = em.load(sb + j); }
    if (hlen) hsum = pm_wave_sum(hsum);
    double run = 0.0;
    double* slot = lds + ebase;
#pragma unroll
    for (int k = 0; k < K; k++) {
      run += v[k];
      if ((int32_t)id[k] < 0) { *slot++ = run; run = 0.0; }
    }
    const double y = pm_scan_seg(run, reach, lane);
    double carry = pm_dpp<0x138, 0xF>(y);   // wave_shr:1 (lane 0 gets 0)
    if (ebase == 0) carry += hsum;
    if (ne) {   // the lane's first end: what the lanes below it hold of that segment comes first in the sum
      const double first = carry + lds[ebase];
      lds[ebase] = first;
      if (heavy && ebase == 0) s.lp[c] = first;
    }
    if (lane == 63) { if (n_ends == 0) { s.lp[c] = y; s.rp[c] = y; } else s.rp[c] = y; }
    if (skip >= n_ends) return;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
    for (int i = 0; i < PRE; i++) { const u32 t = skip + lane + 64 * i; if (t < n_ends) em.finish(sb + t, pre[i], lds[t]); }
    for (u32 t = skip + lane + 64 * PRE; t < n_ends; t += 128) {
      const u32 t1 = t + 64;
      const bool h1 = t1 < n_ends;
      const typename Emit::Ctx x0 = em.load(sb + t), x1 = h1 ? em.load(sb + t1) : x0;
      em.finish(sb + t, x0, lds[t]);
      if (h1) em.finish(sb + t1, x1, lds[t1]);
    }
    return;
  } else {
  u32 ne = 0;
#pragma unroll
  for (int k = 0; k < K; k++) ne += id[k] >> 31;
  const u32 incl = pm_scan_incl(ne);   // segment ends in this and the lower lanes
  const u32 ebase = incl - ne;
  const u32 n_ends = (u32)__builtin_amdgcn_readlane((int)incl, 63);
  const u64 heads = __ballot(ne > 0);
  // (one window unless the chunk holds more segment ends than the wavefront's share of LDS; then the pass is repeated)
  for (u32 w0 = skip; w0 == skip || w0 < n_ends; w0 += PM_LDS_SLOTS) {
    double v[K];
#pragma unroll
    for (int k = 0; k < K; k++) v[k] = src(id[k]);
    double hsum = head_sum();
    typename Emit::Ctx pre[PRE];
#pragma unroll
    for (int i = 0; i < PRE; i++) { const u32 j = w0 + lane + 64 * i; if (j < n_ends) pre[i] = em.load(sb + j); }
    if (hlen) hsum = pm_wave_sum(hsum);
    // lane-local pass in entry order: a segment that ends after an earlier end of the same lane is complete -> staged in LDS
    // at its local index; the sum up to the lane's first end waits for the carry; the open tail feeds the wavefront scan
    double run = 0.0, first_part = 0.0;
    bool got = false;
    u32 j = ebase;
#pragma unroll
    for (int k = 0; k < K; k++) {
      run += v[k];
      if ((int32_t)id[k] < 0) {
        if (!got) { first_part = run; got = true; }
        else if (j >= w0 && j < w0 + PM_LDS_SLOTS) lds[j - w0] = run;
        ++j; run = 0.0;
      }
    }
    double y = run;   // segmented inclusive scan; a lane that holds a segment end starts a new run with its tail
    // lane may add the partial sum of lane - d iff no lane in (lane - d, lane] holds an end, i.e. iff d <= its distance to the
    // nearest end at or below it (the lane itself: 0; none: lane + 1 -- which also covers the lane >= d test)
    const u64 below = heads & ((2ULL << lane) - 1ULL);
    const int reach = below ? lane - (63 - __clzll((long long)below)) : lane + 1;
    y = pm_scan_seg(y, reach, lane);
    double carry = pm_dpp<0x138, 0xF>(y);   // wave_shr:1 (lane 0 gets 0)
    if (ebase == 0) carry += hsum;   // the chunk's first end also gets the re-read head
    if (got && ebase >= w0 && ebase < w0 + PM_LDS_SLOTS) lds[ebase - w0] = carry + first_part;
    if (w0 == skip) {  // partial sums for pm_fix: a chunk without any end lies wholly inside one segment (its sum is both)
      if (lane == 63) { if (n_ends == 0) { s.lp[c] = y; s.rp[c] = y; } else s.rp[c] = y; }
      if (heavy && got && ebase == 0) s.lp[c] = carry + first_part;
    }
    if (w0 >= n_ends) break;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    const u32 wn = min(n_ends - w0, (u32)PM_LDS_SLOTS);
#pragma unroll
    for (int i = 0; i < PRE; i++) { const u32 t = lane + 64 * i; if (t < wn) em.finish(sb + w0 + t, pre[i], lds[t]); }
    for (u32 t = lane + 64 * PRE; t < wn; t += 128) {   // beyond the prefetched contexts: two segments per lane and trip
      const u32 t1 = t + 64;
      const bool h1 = t1 < wn;
      const typename Emit::Ctx x0 = em.load(sb + w0 + t), x1 = h1 ? em.load(sb + w0 + t1) : x0;
      em.finish(sb + w0 + t, x0, lds[t]);
      if (h1) em.finish(sb + w0 + t1, x1, lds[t1]);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  }
  }
}
// a heavy crossing segment that ends in chunk c: right partial of the chunk it started in + the chunks wholly inside it +
// this chunk's left partial, in chunk order; one thread per chunk
template <class Emit>
__device__ __forceinline__ void pm_fix(const PmSide& s, u32 c, const Emit& em) {
  if (c >= s.n_chunks) return;
  const u32 f = s.fix_first[c];
  if (f == PM_NONE) return;
  const u32 seg = s.seg_base[c];
  const typename Emit::Ctx cx = em.load(seg);
  double S = s.rp[f];
  for (u32 k = f + 1; k < c; k++) S += s.lp[k];
  S += s.lp[c];
  em.finish(seg, cx, S);
}
// change counter of the round: one atomic per block
__device__ __forceinline__ void pm_count_changes(int ch, int* lds_ch, EmState* rec) {
  if (threadIdx.x == 0) *lds_ch = 0;
  __syncthreads();
  if (__ballot(ch != 0)) {
    int wsum = ch;
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) wsum += __shfl_down(wsum, d, 64);
    if (lane_id() == 0) atomicAdd(lds_ch, wsum);
  }
  __syncthreads();
  if (threadIdx.x == 0 && *lds_ch) atomicAdd(&rec->chcount, *lds_ch);
}
}  // namespace
