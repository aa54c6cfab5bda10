// kamd_bus.hip -- barcode / UMI technologies on the device (kamd_bus_split, kamd_bus_records): the per-item rules are those of kamd_bustag.h, this file
// is the compaction around them.  Neither call reads or writes the EC state, the counts, the tuple table or the fragment-length sample.
//
//   k_bus_count       one thread per input item: what the lengths of its reads decide (dropped or not, the fields' lengths, the cut's length) -> the
//                     surviving items of the block, the drops, the two length histograms (LDS bins, one global add per non-empty bin and block)
//   k_bus_scan        (kamd_bus_scan.h) one block: exclusive scan of the block counts in place, 256 at a time with a running carry; the total is n_valid
//   k_bus_scatter     one thread per input item again: rank among the block's survivors by ballot -> compact position j; tag, source item, cut length
//   k_bus_cut         BUS_CUT_LANES lanes per compact item: the cut sequence re-packed from base `start`, the lanes of an item writing consecutive words
//                     (a wavefront writes 8 consecutive records); the cut's "has an N" flag is the OR of its mask words over the item's lanes
//   k_rec_count / k_rec_scatter   the same count / scan / scatter over d_ec >= 0 for the 32-byte records; a FOREIGN row stops the scatter
//
// Items keep their input order because thread t of block b takes item 256 b + t and ranks are taken in lane, wavefront and block order.  The passes are
// separate launches on the context stream: nothing waits for another workgroup inside a launch.  Scratch: one u32 per 256 items and the counters.
#include "kamd_dev.h"
#include "kamd_bustag.h"
#include "kamd_bus_scan.h"

namespace {

constexpr int BUS_CUT_LANES = 8;

struct BusCounters {
  u64 n_valid, n_drop_umi, n_drop_bc, n_foreign;
  u64 hist[66];   // barcode lengths 0 .. 32, then UMI lengths 0 .. 32
  u32 max_seq_len, pad;
};

__device__ __forceinline__ kamd::BusLens item_lens(const kamd_bus_layout& L, const uint16_t* __restrict__ lens, u64 i, int max_len, int* l0, int* l1) {
  // (a length beyond max_len cannot come from a packer; clamped so that no index derived from it leaves the record)
  *l0 = min((int)lens[i * L.n_files], max_len);
  *l1 = L.n_files > 1 ? min((int)lens[i * L.n_files + 1], max_len) : 0;
  return kamd::bus_item_lens(L, *l0, *l1);
}

__global__ __launch_bounds__(BLOCK) void k_bus_count(kamd_bus_layout L, const uint16_t* __restrict__ lens, u64 n, int max_len, int seq_max_len, u32* __restrict__ blk_cnt,
                                                     BusCounters* ctr) {
  __shared__ u32 s_hist[66];
  const u64 i = (u64)blockIdx.x * BLOCK + threadIdx.x;
  if (threadIdx.x < 66) s_hist[threadIdx.x] = 0;
  __syncthreads();
  int status = -1;
  u32 seq_len = 0;
  if (i < n) {
    int l0, l1;
    const kamd::BusLens ln = item_lens(L, lens, i, max_len, &l0, &l1);
    status = ln.status;
    if (status != kamd::BUS_ITEM_DROP_UMI && kamd::bus_len_counted(ln.umi_len)) atomicAdd(&s_hist[33 + ln.umi_len], 1u);
    if (status == kamd::BUS_ITEM_OK) {
      if (kamd::bus_len_counted(ln.bc_len)) atomicAdd(&s_hist[ln.bc_len], 1u);
      seq_len = (u32)min(ln.seq_len, seq_max_len);
    }
  }
  const int n_ok = __syncthreads_count(status == kamd::BUS_ITEM_OK);
  const int n_umi = __syncthreads_count(status == kamd::BUS_ITEM_DROP_UMI);
  const int n_bc = __syncthreads_count(status == kamd::BUS_ITEM_DROP_BC);
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) seq_len = max(seq_len, (u32)__shfl_xor((int)seq_len, d, 64));
  if (lane_id() == 0 && seq_len) atomicMax(&ctr->max_seq_len, seq_len);
  if (threadIdx.x < 66 && s_hist[threadIdx.x]) atomicAdd(&ctr->hist[threadIdx.x], (u64)s_hist[threadIdx.x]);
  if (threadIdx.x == 0) {
    blk_cnt[blockIdx.x] = (u32)n_ok;
    if (n_umi) atomicAdd(&ctr->n_drop_umi, (u64)n_umi);
    if (n_bc) atomicAdd(&ctr->n_drop_bc, (u64)n_bc);
  }
}

__global__ __launch_bounds__(BLOCK) void k_bus_scatter(kamd_bus_layout L, const u32* __restrict__ words, const uint16_t* __restrict__ lens, u64 n, int max_len,
                                                       int seq_words, int rec_words, int seq_max_len, const u32* __restrict__ blk_off,
                                                       kamd_bus_tag* __restrict__ tags, u32* __restrict__ src, uint16_t* __restrict__ seq_len) {
  __shared__ u32 s_w[BUS_WAVES];
  const u64 i = (u64)blockIdx.x * BLOCK + threadIdx.x;
  bool valid = false;
  kamd::BusLens ln{};
  int l0 = 0, l1 = 0;
  if (i < n) { ln = item_lens(L, lens, i, max_len, &l0, &l1); valid = ln.status == kamd::BUS_ITEM_OK; }
  const u32 rank = block_rank(valid, s_w);
  if (!valid) return;
  const u64 j = (u64)blk_off[blockIdx.x] + rank;   // (j <= i < n: inside the caller's [n_items] buffers)
  const u32* rec = words + i * (u64)L.n_files * rec_words;
  const kamd::BusItemView it{{rec, L.n_files > 1 ? rec + rec_words : rec}, {l0, l1}, seq_words};
  tags[j] = kamd::bus_item_tag(L, it, ln);
  src[j] = (u32)i;
  seq_len[j] = (uint16_t)min(ln.seq_len, seq_max_len);
}

__global__ __launch_bounds__(BLOCK) void k_bus_cut(kamd_bus_layout L, const u32* __restrict__ words, int seq_words, int rec_words, const u64* __restrict__ n_valid,
                                                   const u32* __restrict__ src, const uint16_t* __restrict__ seq_len, int out_seq_words, int out_rec_words,
                                                   u32* __restrict__ out_words) {
  const u64 t = (u64)blockIdx.x * BLOCK + threadIdx.x, j = t / BUS_CUT_LANES;
  const int sub = (int)(t % BUS_CUT_LANES);
  if (j >= *n_valid) return;   // (the BUS_CUT_LANES lanes of an item leave together)
  const u32* rec = words + ((u64)src[j] * L.n_files + L.seq.file) * rec_words;
  const u32* rec_mask = rec + seq_words;
  const int mask_words = rec_words - seq_words, out_mask_words = out_rec_words - out_seq_words;
  const int start = L.seq.start, len = (int)seq_len[j];
  u32 any = 0;
  for (int w = sub; w < out_mask_words; w += BUS_CUT_LANES) any |= kamd::bus_cut_mask_word(rec_mask, mask_words, start, len, w);
#pragma unroll
  for (int d = 1; d < BUS_CUT_LANES; d <<= 1) any |= (u32)__shfl_xor((int)any, d, BUS_CUT_LANES);
  u32* out = out_words + j * (u64)out_rec_words;
  for (int x = sub; x < out_rec_words; x += BUS_CUT_LANES) {
    u32 v;
    if (x < out_seq_words - 1) v = kamd::bus_cut_seq_word(rec, seq_words, start, len, x);
    else if (x == out_seq_words - 1) v = any ? kamd::REC_FLAG_HAS_N : 0u;
    else v = kamd::bus_cut_mask_word(rec_mask, mask_words, start, len, x - out_seq_words);
    out[x] = v;
  }
}

__global__ __launch_bounds__(BLOCK) void k_rec_count(const int32_t* __restrict__ ec, u64 n, u32* __restrict__ blk_cnt, BusCounters* ctr) {
  const u64 i = (u64)blockIdx.x * BLOCK + threadIdx.x;
  const int32_t e = i < n ? ec[i] : KAMD_READ_EC_NONE;
  const int n_ok = __syncthreads_count(e >= 0);
  const int n_foreign = __syncthreads_count(e < 0 && e != KAMD_READ_EC_NONE);   // (any negative row but NONE: nothing a record could name)
  if (threadIdx.x == 0) {
    blk_cnt[blockIdx.x] = (u32)n_ok;
    if (n_foreign) atomicAdd(&ctr->n_foreign, (u64)n_foreign);
  }
}

__global__ __launch_bounds__(BLOCK) void k_rec_scatter(const kamd_bus_tag* __restrict__ tags, const int32_t* __restrict__ ec, u64 n, const u32* __restrict__ blk_off,
                                                       const BusCounters* __restrict__ ctr, kamd_bus_record* __restrict__ out) {
  __shared__ u32 s_w[BUS_WAVES];
  if (ctr->n_foreign) return;   // (uniform: no record is written for a batch that holds a foreign row)
  const u64 i = (u64)blockIdx.x * BLOCK + threadIdx.x;
  const int32_t e = i < n ? ec[i] : KAMD_READ_EC_NONE;
  const u32 rank = block_rank(e >= 0, s_w);
  if (e < 0) return;
  const kamd_bus_tag t = tags[i];
  kamd_bus_record r;
  r.barcode = t.barcode; r.umi = t.umi; r.ec = e; r.count = 1; r.flags = t.flags; r.pad = 0;
  out[(u64)blk_off[blockIdx.x] + rank] = r;
}

int bus_prepare(kamd_ctx* c, u64 n) {
  HIPC(hipSetDevice(c->device));
  for (hipEvent_t& e : c->bus_ev) if (!e) HIPC(hipEventCreate(&e));
  if (int rc = c->bus_blk.ensure(std::max<u64>(grid_for(n, BLOCK), 1) * sizeof(u32), 0, c->stream)) return rc;
  if (int rc = c->bus_ctr.ensure(sizeof(BusCounters), 0, c->stream)) return rc;
  HIPC(hipMemsetAsync(c->bus_ctr.p, 0, sizeof(BusCounters), c->stream));
  HIPC(hipEventRecord(c->bus_ev[0], c->stream));
  return 0;
}
int bus_finish(kamd_ctx* c, BusCounters* ctr, float* ms) {
  HIPC(hipGetLastError());
  HIPC(hipEventRecord(c->bus_ev[1], c->stream));
  HIPC(hipMemcpyAsync(ctr, c->bus_ctr.p, sizeof *ctr, hipMemcpyDeviceToHost, c->stream));
  HIPC(hipStreamSynchronize(c->stream));
  HIPC(hipEventElapsedTime(ms, c->bus_ev[0], c->bus_ev[1]));
  return 0;
}

}  // namespace

extern "C" int kamd_bus_split(kamd_ctx* c, const kamd_bus_layout* L, const uint32_t* d_words, const uint16_t* d_len, uint64_t n_items, int32_t max_len,
                              kamd_bus_tag* d_tags, uint32_t* d_src, uint32_t* d_seq_words, uint16_t* d_seq_len, int32_t seq_max_len,
                              kamd_bus_split_stats* out) {
  if (!c || !L) return kamd::fail(-1, "kamd_bus_split: null argument");
  char why[256];
  if (kamd::bus_layout_check(L, why, sizeof why)) return kamd::fail(-1, std::string("kamd_bus_split: ") + why);
  if (max_len <= 0 || max_len > 65535) return kamd::fail(-1, "kamd_bus_split: max_len must be in [1, 65535]");
  if (seq_max_len > 65535 || seq_max_len < kamd_bus_seq_max_len(L, max_len))
    return kamd::fail(-1, "kamd_bus_split: seq_max_len must be in [kamd_bus_seq_max_len(layout, max_len), 65535]");
  if (n_items >= 0xFFFFFFFFULL) return kamd::fail(-1, "kamd_bus_split: a batch holds fewer than 2^32 - 1 items");
  if (out) { memset(out, 0, sizeof *out); out->n_items = n_items; }
  if (n_items == 0) return 0;
  if (!d_words || !d_len || !d_tags || !d_src || !d_seq_words || !d_seq_len) return kamd::fail(-1, "kamd_bus_split: null argument");
  if (int rc = bus_prepare(c, n_items)) return rc;
  const int seq_words = (max_len + 15) / 16 + 1, rec_words = (int)kamd_packed_record_words(max_len);
  const int out_seq_words = (seq_max_len + 15) / 16 + 1, out_rec_words = (int)kamd_packed_record_words(seq_max_len);
  const unsigned nb = grid_for(n_items, BLOCK);
  u32* blk = c->bus_blk.as<u32>();
  BusCounters* ctr = c->bus_ctr.as<BusCounters>();
  hipLaunchKernelGGL(k_bus_count, dim3(nb), dim3(BLOCK), 0, c->stream, *L, d_len, (u64)n_items, (int)max_len, (int)seq_max_len, blk, ctr);
  hipLaunchKernelGGL(k_bus_scan, dim3(1), dim3(BLOCK), 0, c->stream, blk, (u64)nb, &ctr->n_valid);
  hipLaunchKernelGGL(k_bus_scatter, dim3(nb), dim3(BLOCK), 0, c->stream, *L, (const u32*)d_words, d_len, (u64)n_items, (int)max_len, seq_words, rec_words, (int)seq_max_len,
                     (const u32*)blk, d_tags, (u32*)d_src, d_seq_len);
  hipLaunchKernelGGL(k_bus_cut, dim3(grid_for(n_items * BUS_CUT_LANES, BLOCK)), dim3(BLOCK), 0, c->stream, *L, (const u32*)d_words, seq_words, rec_words,
                     (const u64*)&ctr->n_valid, (const u32*)d_src, (const uint16_t*)d_seq_len, out_seq_words, out_rec_words, (u32*)d_seq_words);
  BusCounters h{};
  float ms = 0.f;
  if (int rc = bus_finish(c, &h, &ms)) return rc;
  if (out) {
    out->n_valid = h.n_valid; out->n_dropped_umi = h.n_drop_umi; out->n_dropped_bc = h.n_drop_bc;
    for (int i = 0; i < 33; i++) { out->bc_len_hist[i] = h.hist[i]; out->umi_len_hist[i] = h.hist[33 + i]; }
    out->max_seq_len = (int32_t)h.max_seq_len; out->last_ms = ms;
  }
  return 0;
}

extern "C" int kamd_bus_records(kamd_ctx* c, const kamd_bus_tag* d_tags, const int32_t* d_ec, uint64_t n, kamd_bus_record* d_out, uint64_t* n_out) {
  if (!c) return kamd::fail(-1, "kamd_bus_records: null context");
  if (n_out) *n_out = 0;
  if (n >= 0xFFFFFFFFULL) return kamd::fail(-1, "kamd_bus_records: a batch holds fewer than 2^32 - 1 items");
  if (n == 0) return 0;
  if (!d_tags || !d_ec || !d_out) return kamd::fail(-1, "kamd_bus_records: null argument");
  if (int rc = bus_prepare(c, n)) return rc;
  const unsigned nb = grid_for(n, BLOCK);
  u32* blk = c->bus_blk.as<u32>();
  BusCounters* ctr = c->bus_ctr.as<BusCounters>();
  hipLaunchKernelGGL(k_rec_count, dim3(nb), dim3(BLOCK), 0, c->stream, d_ec, (u64)n, blk, ctr);
  hipLaunchKernelGGL(k_bus_scan, dim3(1), dim3(BLOCK), 0, c->stream, blk, (u64)nb, &ctr->n_valid);
  hipLaunchKernelGGL(k_rec_scatter, dim3(nb), dim3(BLOCK), 0, c->stream, d_tags, d_ec, (u64)n, (const u32*)blk, (const BusCounters*)ctr, d_out);
  BusCounters h{};
  float ms = 0.f;
  if (int rc = bus_finish(c, &h, &ms)) return rc;
  if (h.n_foreign)
    return kamd::fail(-4, "kamd_bus_records: " + std::to_string(h.n_foreign) + " items carry KAMD_READ_EC_FOREIGN: their batch is not part of the finalized EC result; no record written");
  if (n_out) *n_out = h.n_valid;
  return 0;
}
