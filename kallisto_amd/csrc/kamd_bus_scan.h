// kamd_bus_scan.h -- the two pieces every count / scan / scatter compaction of kamd_bus.hip and kamd_bussort.hip is made of (a copy per unit).
#pragma once

#include "kamd_dev.h"

namespace {

constexpr int BUS_WAVES = BLOCK / 64;

// rank of a thread's item among the block's items with `valid`, in thread order
__device__ __forceinline__ u32 block_rank(bool valid, u32* s_w) {
  const u64 b = __ballot(valid);
  const int lane = lane_id(), wave = threadIdx.x >> 6;
  if (lane == 0) s_w[wave] = (u32)__popcll(b);
  __syncthreads();
  u32 off = 0;
  for (int w = 0; w < wave; w++) off += s_w[w];
  return off + (u32)__popcll(b & ((1ULL << lane) - 1ULL));
}

// row blockIdx.x of blk[gridDim.x][nb]: counts -> exclusive offsets, in place; total[blockIdx.x] = their sum.  (One block: one array.)
__global__ __launch_bounds__(BLOCK) void k_bus_scan(u32* __restrict__ blk, u64 nb, u64* total) {
  __shared__ u32 s_w[BUS_WAVES];
  __shared__ u32 s_carry;
  const int lane = lane_id(), wave = threadIdx.x >> 6;
  blk += (u64)blockIdx.x * nb;
  if (threadIdx.x == 0) s_carry = 0;
  __syncthreads();
  for (u64 base = 0; base < nb; base += BLOCK) {   // (nb is uniform: every thread makes every trip)
    const u64 i = base + threadIdx.x;
    const u32 v = i < nb ? blk[i] : 0u;
    const u32 incl = wave_incl_scan(v);
    if (lane == 63) s_w[wave] = incl;
    __syncthreads();
    u32 woff = 0, tot = 0;
    for (int w = 0; w < BUS_WAVES; w++) { if (w < wave) woff += s_w[w]; tot += s_w[w]; }
    const u32 carry = s_carry;
    if (i < nb) blk[i] = carry + woff + incl - v;
    __syncthreads();
    if (threadIdx.x == 0) s_carry = carry + tot;
    __syncthreads();
  }
  if (threadIdx.x == 0) total[blockIdx.x] = s_carry;
}

}  // namespace
