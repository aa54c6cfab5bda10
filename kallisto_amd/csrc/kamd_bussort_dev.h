// kamd_bussort_dev.h -- what kamd_bussort.hip and kamd_busgenes.hip share on the device side: the counters of a call, a record as two 16-byte halves,
// the heads of barcodes and groups with their two kernels (k_cnt_heads, k_cnt_starts), the collapsed unit records as entries (k_cnt_entries) -- a
// copy per unit, as kamd_bus_scan.h -- and the host functions of kamd_bussort.hip that the other unit calls.
#pragma once

#include "kamd_dev.h"
#include "kamd_bussort.h"
#include "kamd_bus_scan.h"

namespace kamdi {
struct SortCounters {
  u64 n_bad, n_out, n_over;                                                    // kamd_bus_sort
  u64 n_unsorted, n_barcodes, n_groups, n_units, n_multi_rec, n_multi_grp;     // kamd_bus_count
  u32 or_w[kamd::BUS_KEY_WORDS], and_w[kamd::BUS_KEY_WORDS];
};
// kamd_bussort.hip: the sort of kamd_bus_sort (two synchronisations; `who` begins the error texts), the counters' read-back (one synchronisation),
// the two events around a call
int bus_sort_records(kamd_ctx* c, kamd_bus_record* d_rec, u64 n, const int32_t* d_map, u64 n_map, int collapse, u64* n_out, kamd_bus_sort_stats* st, const std::string& who);
int bus_read_counters(kamd_ctx* c, SortCounters* h);
int bus_events_begin(kamd_ctx* c);
int bus_events_end(kamd_ctx* c, float* ms);
}  // namespace kamdi

namespace {

struct RecQ { uint4 a, b; };   // a record as its two 16-byte halves
__device__ __forceinline__ RecQ load_rec(const kamd_bus_record* p) {
  const uint4* q = reinterpret_cast<const uint4*>(p);
  RecQ x; x.a = q[0]; x.b = q[1];
  return x;
}
__device__ __forceinline__ void store_rec(kamd_bus_record* p, const RecQ& x) {
  uint4* q = reinterpret_cast<uint4*>(p);
  q[0] = x.a; q[1] = x.b;
}
__device__ __forceinline__ kamd_bus_record rec_of(const RecQ& x) {
  kamd_bus_record r;
  r.barcode = (u64)x.a.x | ((u64)x.a.y << 32); r.umi = (u64)x.a.z | ((u64)x.a.w << 32);
  r.ec = (int32_t)x.b.x; r.count = x.b.y; r.flags = x.b.z; r.pad = x.b.w;
  return r;
}
__device__ __forceinline__ RecQ q_of(const kamd_bus_record& r) {
  RecQ x;
  x.a = make_uint4((u32)r.barcode, (u32)(r.barcode >> 32), (u32)r.umi, (u32)(r.umi >> 32));
  x.b = make_uint4((u32)r.ec, r.count, r.flags, r.pad);
  return x;
}
__device__ __forceinline__ kamd_bus_record get_rec(const kamd_bus_record* p) { return rec_of(load_rec(p)); }

// ---- kamd_bus_count ----
struct Heads { bool bc, grp, unsorted; };
__device__ __forceinline__ Heads rec_heads(const kamd_bus_record* rec, u64 i, u64 n, kamd_bus_record* me) {
  Heads h{false, false, false};
  if (i >= n) return h;
  *me = get_rec(rec + i);
  if (i == 0) { h.bc = h.grp = true; return h; }
  const kamd_bus_record p = get_rec(rec + i - 1);
  h.bc = !kamd::bus_same_barcode(p, *me);
  h.grp = !kamd::bus_same_group(p, *me);
  h.unsorted = kamd::bus_key_less(*me, p);
  return h;
}

__global__ __launch_bounds__(BLOCK) void k_cnt_heads(const kamd_bus_record* __restrict__ rec, u64 n, u32* __restrict__ blk_bc, u32* __restrict__ blk_grp, SortCounters* ctr) {
  const u64 i = (u64)blockIdx.x * BLOCK + threadIdx.x;
  kamd_bus_record me;
  const Heads h = rec_heads(rec, i, n, &me);
  const int n_bc = __syncthreads_count(h.bc), n_grp = __syncthreads_count(h.grp), n_uns = __syncthreads_count(h.unsorted);
  if (threadIdx.x == 0) {
    blk_bc[blockIdx.x] = (u32)n_bc;
    blk_grp[blockIdx.x] = (u32)n_grp;
    if (n_uns) atomicAdd(&ctr->n_unsorted, (u64)n_uns);
  }
}

__global__ __launch_bounds__(BLOCK) void k_cnt_starts(const kamd_bus_record* __restrict__ rec, u64 n, const u32* __restrict__ blk_bc, const u32* __restrict__ blk_grp,
                                                      const SortCounters* __restrict__ ctr, u64* __restrict__ barcodes, u32* __restrict__ gstart) {
  __shared__ u32 s_w[2][BUS_WAVES];
  if (ctr->n_unsorted) return;   // (uniform)
  const u64 i = (u64)blockIdx.x * BLOCK + threadIdx.x;
  kamd_bus_record me;
  const Heads h = rec_heads(rec, i, n, &me);
  const u32 r_bc = block_rank(h.bc, s_w[0]), r_grp = block_rank(h.grp, s_w[1]);
  if (h.bc) barcodes[(u64)blk_bc[blockIdx.x] + r_bc] = me.barcode;   // (fewer heads than records: inside [n])
  if (h.grp) gstart[(u64)blk_grp[blockIdx.x] + r_grp] = (u32)i;
  if (i == 0) gstart[ctr->n_groups] = (u32)n;                       // (n_groups <= n: inside [n + 1])
}

__global__ __launch_bounds__(BLOCK) void k_cnt_entries(const kamd_bus_record* __restrict__ units, u64 n, kamd_bus_entry* __restrict__ out) {
  const u64 j = (u64)blockIdx.x * BLOCK + threadIdx.x;
  if (j >= n) return;
  const kamd_bus_record r = get_rec(units + j);
  kamd_bus_entry e;
  e.row = r.pad; e.ec = r.ec; e.value = r.count;
  out[j] = e;
}

}  // namespace
