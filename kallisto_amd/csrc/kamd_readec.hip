// kamd_readec.hip -- per-read equivalence classes (kamd_read_ecs): a second pass over a batch, after kamd_ec_finalize, that recomputes every item's
// transcript set and looks it up in the finalized result.  Nothing here writes the EC state; the kernels of kamd_match.hip / kamd_ec.hip are not involved.
//
//   k_rec_table_build   one thread per row of the finalized CSR: the row's tag, one compare-and-swap into the table (kamd_readec.h).  Once per result.
//   k_read_ecs<PAIRED>  one thread per item, what k_pseudoalign_overflow and k_explicit_write do for one item (match_mate per mate, pair_is_mapped,
//                       item_filter_cfg / first_hit / keep_transcript over for_each_member, HitBlocks with the per-hit strand filter), but the members
//                       go into the look-up of kamd_readec.h instead of a record: enumerated once for size and tag, once more per candidate slot.
//
// Scratch is bounded independently of n_items.  A call works through its batch in chunks of REC_CHUNK items; per chunk
//   first tier    every item with a list of REC_CAP_SMALL set ids: REC_CHUNK x (2 x 64 [+ EXPLICIT_HITS with the per-hit strand filter]) words
//                 = 32 MiB (96 MiB with that filter);
//   second tier   the items whose list overflowed (listed by the first launch, at most REC_CHUNK of them) are re-run with TUPLE_CAP_BIG entries by
//                 REC_BIG_THREADS threads that take the listed items in turn: REC_BIG_THREADS x (2 x 1024 + EXPLICIT_HITS) words = 36 MiB;
// plus 4 bytes per item of a chunk for the list and the table itself (16 bytes x the power of two >= 2 x n_ecs).  The second launch reads the
// length of its list from device memory, so a call synchronises the stream once, at its end.
// Every loop is bounded: a probe by the table's capacity, a list by its cap, the second tier's item loop by the chunk; nothing waits for another thread.
#include "kamd_dev.h"
#include "kamd_readec.h"

namespace {

constexpr u64 REC_CHUNK = 65536;
constexpr int REC_CAP_SMALL = 64;
constexpr u32 REC_BIG_THREADS = 4096;

struct RecCounters { u64 n_mapped, n_none, n_foreign, n_hit_overflow, n_list_overflow, n_second; u32 n_big, pad; };

__global__ __launch_bounds__(BLOCK) void k_rec_table_build(const u64* __restrict__ ec_off, const u32* __restrict__ ec_ids, u64 n_ecs, kamd::RecTable t, u64* n_fail) {
  const u64 r = (u64)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n_ecs) return;
  const bool ok = kamd::rectable_insert_row(t, (const uint64_t*)ec_off, ec_ids, r,
                                            [](uint64_t* p, uint64_t expect, uint64_t want) { return (uint64_t)atomicCAS((u64*)p, (u64)expect, (u64)want); });
  if (!ok) atomicAdd(n_fail, 1ULL);
}

// items == nullptr: the chunk's items 0 .. n-1, one per thread (first tier; an item whose list overflows is appended to big_items);
// items != nullptr: the *n_dev listed items, taken in turn by the threads of the grid (second tier; big_items == nullptr)
template <bool PAIRED>
__global__ __launch_bounds__(BLOCK) void k_read_ecs(DevIndex ix, const u32* __restrict__ words, const uint16_t* __restrict__ lens, const u32* __restrict__ items,
                                                     u64 n, const u32* __restrict__ n_dev, int seq_words, int rec_words, u32* scratch, int cap, int hit_cap,
                                                     FilterDev fd, int filter, kamd::RecTable tab, const u64* __restrict__ res_off,
                                                     const u32* __restrict__ res_ids, int32_t* d_ec, u32* big_items, RecCounters* ctr) {
  const u64 tid = (u64)blockIdx.x * blockDim.x + threadIdx.x, n_threads = (u64)gridDim.x * blockDim.x;
  if (items) n = *n_dev;
  u32 s_mapped = 0, s_none = 0, s_foreign = 0, s_hit = 0, s_list = 0, s_second = 0;
  const int item_words = rec_words * (PAIRED ? 2 : 1);
  // scratch of a thread: the list (cap words), the cursors of the --union merge (cap), the distinct block / strand pairs of mate 1's hits (hit_cap)
  u32* sbase = scratch + tid * (u64)(2 * cap + hit_cap);
  const kamd::Table t = make_table(ix, !PAIRED);
  const kamd::PosTables pt = pos_tables(ix);
  for (u64 i = tid; i < n; i += n_threads) {   // (first tier: the grid covers the chunk, one trip)
    const u64 item = items ? items[i] : i;
    if (items) ++s_second;
    kamd::EcList ecs; ecs.e = sbase; ecs.cap = cap; ecs.n = 0; ecs.overflow = false;
    u32* cur = sbase + cap;
    kamd::HitBlocks hb{ix.slot_block, sbase + 2 * cap, hit_cap, 0, false};
    kamd::MateInfo m0, m1; m1.n_hits = 0; m1.n_nonempty = 0; m1.first_slot = 0; m1.first_pos = -1; m1.first_strand = false;
    const u32* rec = words + item * item_words;
    kamd::ReadView r0{rec, rec + seq_words, PAIRED ? (int)lens[2 * item] : (int)lens[item]};
    kamd::match_mate(t, ix.uec_ec, ix.ec_nonempty, r0, ix.k, ecs, m0, ix.union_mode ? kamd::EC_MATE1 : 0u, hit_cap ? &hb : nullptr);
    if (PAIRED) {
      kamd::ReadView r1{rec + rec_words, rec + rec_words + seq_words, (int)lens[2 * item + 1]};
      kamd::match_mate(t, ix.uec_ec, ix.ec_nonempty, r1, ix.k, ecs, m1, ix.union_mode ? kamd::EC_MATE2 : 0u);
    }
    if (ecs.overflow) {
      if (big_items) big_items[atomicAdd(&ctr->n_big, 1u)] = (u32)item;   // (at most n entries: one per item of the chunk)
      else { ++s_list; d_ec[item] = KAMD_READ_EC_NONE; }
      continue;
    }
    int32_t row = KAMD_READ_EC_NONE;
    if (kamd::pair_is_mapped(m0, m1)) {
      kamd::FilterCfg cfg = item_filter_cfg(fd, PAIRED, m0, m1);
      const bool filt = filter && (cfg.fraglen || cfg.strand);
      bool bad = false;
      if (filt && needs_hit_list(fd, m1)) {   // the per-hit strand filter with mate 2 without hits: every hit of mate 1 decides
        cfg.hits1 = hb.e; cfg.n_hits1 = hb.n;
        if (hb.overflow) { bad = true; ++s_hit; }
      }
      if (!bad) {
        const kamd::FirstHit h0 = first_hit(ix, m0), h1 = first_hit(ix, m1);
        row = kamd::rectable_lookup(tab, (const uint64_t*)res_off, res_ids, [&](auto&& f) {
          for_each_member(ix, ecs, cur, [&](u32 tr) { if (!filt || kamd::keep_transcript(pt, cfg, h0, h1, tr)) f(tr); });
        });
      }
    }
    d_ec[item] = row;
    if (row >= 0) ++s_mapped; else if (row == KAMD_READ_EC_FOREIGN) ++s_foreign; else ++s_none;
  }
  // one set of atomics per wavefront (every lane arrives here)
  const u64 w_mapped = wave_sum64(s_mapped), w_none = wave_sum64(s_none), w_foreign = wave_sum64(s_foreign), w_hit = wave_sum64(s_hit), w_list = wave_sum64(s_list), w_second = wave_sum64(s_second);
  if (lane_id() == 0) {
    if (w_mapped) atomicAdd(&ctr->n_mapped, w_mapped);
    if (w_none) atomicAdd(&ctr->n_none, w_none);
    if (w_foreign) atomicAdd(&ctr->n_foreign, w_foreign);
    if (w_hit) atomicAdd(&ctr->n_hit_overflow, w_hit);
    if (w_list) atomicAdd(&ctr->n_list_overflow, w_list);
    if (w_second) atomicAdd(&ctr->n_second, w_second);
  }
}

int rec_table_ensure(kamd_ctx* c) {
  if (c->rec_table_cap && c->rec_table_gen == c->ec_generation) return 0;
  c->rec_table_cap = 0;
  const u64 n_ecs = c->result.n_ecs, cap = kamd::rectable_capacity(n_ecs);
  if (int rc = c->rec_table.ensure(cap * 16, 0, c->stream)) return rc;
  HIPC(hipMemsetAsync(c->rec_table.p, 0, cap * 16, c->stream));
  if (n_ecs) {
    const kamd::RecTable t{c->rec_table.as<uint64_t>(), cap, ~0ULL};
    hipLaunchKernelGGL(k_rec_table_build, dim3(grid_for(n_ecs, BLOCK)), dim3(BLOCK), 0, c->stream, (const u64*)c->result.d_ec_off, c->result.d_ec_ids, n_ecs, t,
                       &c->rec_ctr.as<RecCounters>()->n_list_overflow);   // (no slot left: cannot happen at this capacity; reported with the call's other errors)
    HIPC(hipGetLastError());
  }
  c->rec_table_cap = cap; c->rec_table_gen = c->ec_generation;
  return 0;
}

template <bool PAIRED>
int read_ecs_chunks(kamd_ctx* c, const DevIndex& ix, const FilterDev& fd, bool filter, const u32* d_words, const uint16_t* d_len, u64 n_items, int seq_words, int rec_words,
                    int32_t* d_ec) {
  const u64 chunk = c->rec_chunk ? c->rec_chunk : REC_CHUNK;
  const int hit_cap = (fd.comprehensive && fd.strand) ? EXPLICIT_HITS : 0;
  const int small_cap = c->rec_small_cap ? c->rec_small_cap : REC_CAP_SMALL;
  const u64 small_words = (u64)(2 * small_cap + hit_cap), big_words = (u64)(2 * TUPLE_CAP_BIG + hit_cap);
  const u64 chunk_max = std::min(chunk, n_items);
  const u64 small_threads = (u64)grid_for(chunk_max, BLOCK) * BLOCK;
  if (int rc = c->rec_scratch.ensure(small_threads * small_words * sizeof(u32), 0, c->stream)) return rc;
  if (int rc = c->rec_big_scratch.ensure((u64)REC_BIG_THREADS * big_words * sizeof(u32), 0, c->stream)) return rc;
  if (int rc = c->rec_big_items.ensure(chunk_max * sizeof(u32), 0, c->stream)) return rc;
  const kamd::RecTable tab{c->rec_table.as<uint64_t>(), c->rec_table_cap, ~0ULL};
  RecCounters* ctr = c->rec_ctr.as<RecCounters>();
  const u64* res_off = (const u64*)c->result.d_ec_off;
  const u32* res_ids = c->result.d_ec_ids;
  const u64 item_words = (u64)rec_words * (PAIRED ? 2 : 1);
  for (u64 first = 0; first < n_items; first += chunk) {
    const u64 n = std::min(chunk, n_items - first);
    const u32* w = d_words + first * item_words;
    const uint16_t* l = d_len + first * (PAIRED ? 2 : 1);
    HIPC(hipMemsetAsync(&ctr->n_big, 0, sizeof(u32), c->stream));
    hipLaunchKernelGGL(k_read_ecs<PAIRED>, dim3(grid_for(n, BLOCK)), dim3(BLOCK), 0, c->stream, ix, w, l, (const u32*)nullptr, n, (const u32*)nullptr, seq_words, rec_words,
                       c->rec_scratch.as<u32>(), small_cap, hit_cap, fd, filter ? 1 : 0, tab, res_off, res_ids, d_ec + first, c->rec_big_items.as<u32>(), ctr);
    HIPC(hipGetLastError());
    hipLaunchKernelGGL(k_read_ecs<PAIRED>, dim3(REC_BIG_THREADS / BLOCK), dim3(BLOCK), 0, c->stream, ix, w, l, (const u32*)c->rec_big_items.as<u32>(), 0ULL,
                       (const u32*)&ctr->n_big, seq_words, rec_words, c->rec_big_scratch.as<u32>(), TUPLE_CAP_BIG, hit_cap, fd, filter ? 1 : 0, tab, res_off, res_ids,
                       d_ec + first, (u32*)nullptr, ctr);
    HIPC(hipGetLastError());
  }
  return 0;
}

}  // namespace

extern "C" int kamd_read_ecs(kamd_ctx* c, const kamd_quant_opts* o, const uint32_t* d_words, const uint16_t* d_len, uint64_t n_items, int32_t max_len,
                             int32_t* d_ec, kamd_read_ecs_stats* out) {
  if (!c || !o) return kamd::fail(-1, "kamd_read_ecs: null argument");
  if (!c->has_index) return kamd::fail(-1, "kamd_read_ecs: no index uploaded");
  if (!c->finalized) return kamd::fail(-1, "kamd_read_ecs: no EC result (call kamd_ec_finalize or kamd_ec_upload first)");
  if (!o->paired && !(o->fld > 0.0 && o->sd > 0.0))
    return kamd::fail(-1, "kamd_read_ecs: fragment length mean and sd must be supplied for single-end reads (-l, -s)");
  if (o->strand < 0 || o->strand > 2) return kamd::fail(-1, "kamd_read_ecs: bad strand option");
  if (!o->paired && o->do_union && !o->single_overhang) return kamd::fail(-5, "kamd_read_ecs: --single with --union needs --single-overhang");
  if (c->ix.n_shades && o->fld != 0.0 && !o->single_overhang)
    return kamd::fail(-5, "kamd_read_ecs: an index with shades cannot take the positional fragment-length filter (-l / -s without --single-overhang)");
  if (max_len <= 0 || max_len > 65535) return kamd::fail(-1, "kamd_read_ecs: max_len must be in [1, 65535]");
  if (c->result.n_ecs >= 0x7FFFFFFFULL) return kamd::fail(-1, "kamd_read_ecs: the EC result has more rows than a 32-bit id holds");
  if (out) { memset(out, 0, sizeof *out); out->n_items = n_items; }
  if (n_items == 0) return 0;
  if (!d_words || !d_len || !d_ec) return kamd::fail(-1, "kamd_read_ecs: null argument");
  HIPC(hipSetDevice(c->device));
  // the options of this call in a copy of the index view (what apply_quant_opts leaves in the context for kamd_pseudoalign; the context's stay as they are)
  DevIndex ix = c->ix;
  ix.no_jump = o->no_jump ? 1 : 0; ix.union_mode = o->do_union ? 1 : 0;
  ix.comprehensive = (o->strand != 0 && (o->no_jump || o->do_union || ix.n_shades)) ? 1 : 0;
  const int seq_words = (max_len + 15) / 16 + 1;
  const int rec_words = (int)kamd_packed_record_words(max_len);
  // the positional filters as kamd_pseudoalign sets them up (has_mean_fl by -l only, fl = (int) of the -l value)
  FilterDev fd{o->single_overhang, o->fld != 0.0 ? 1 : 0, 0, o->strand, ix.comprehensive};
  if (fd.has_mean_fl) fd.fl = (int)o->fld;
  const bool filter = fd.strand != 0 || (!fd.single_overhang && fd.has_mean_fl);
  for (hipEvent_t& e : c->rec_ev) if (!e) HIPC(hipEventCreate(&e));
  if (int rc = c->rec_ctr.ensure(sizeof(RecCounters), 0, c->stream)) return rc;
  HIPC(hipMemsetAsync(c->rec_ctr.p, 0, sizeof(RecCounters), c->stream));
  HIPC(hipEventRecord(c->rec_ev[0], c->stream));
  if (int rc = rec_table_ensure(c)) return rc;
  HIPC(hipEventRecord(c->rec_ev[1], c->stream));
  if (int rc = o->paired ? read_ecs_chunks<true>(c, ix, fd, filter, d_words, d_len, n_items, seq_words, rec_words, d_ec)
                         : read_ecs_chunks<false>(c, ix, fd, filter, d_words, d_len, n_items, seq_words, rec_words, d_ec)) return rc;
  HIPC(hipEventRecord(c->rec_ev[2], c->stream));
  RecCounters ctr{};
  HIPC(hipMemcpyAsync(&ctr, c->rec_ctr.p, sizeof ctr, hipMemcpyDeviceToHost, c->stream));
  HIPC(hipStreamSynchronize(c->stream));
  HIPC(hipEventElapsedTime(&c->rec_table_ms, c->rec_ev[0], c->rec_ev[1]));
  HIPC(hipEventElapsedTime(&c->rec_items_ms, c->rec_ev[1], c->rec_ev[2]));
  if (ctr.n_hit_overflow) return kamd::fail(-4, "kamd_read_ecs: a read's hits touch more blocks than the per-hit strand filter keeps");
  if (ctr.n_list_overflow) return kamd::fail(-4, "kamd_read_ecs: a read's hits carry more distinct transcript sets than the second tier's list keeps");
  c->rec_second = ctr.n_second;
  if (out) { out->n_mapped = ctr.n_mapped; out->n_none = ctr.n_none; out->n_foreign = ctr.n_foreign; out->last_ms = c->rec_table_ms + c->rec_items_ms; }
  return 0;
}

extern "C" int kamd_debug_read_ecs(kamd_ctx* c, uint64_t chunk_items, int32_t list_cap, float* table_ms, float* items_ms, uint64_t* n_second_tier) {
  if (!c) return kamd::fail(-1, "kamd_debug_read_ecs: null context");
  if (chunk_items > 0xFFFFFFFFULL) return kamd::fail(-1, "kamd_debug_read_ecs: a chunk holds at most 2^32 - 1 items");
  if (list_cap < 0 || list_cap > TUPLE_CAP_BIG) return kamd::fail(-1, "kamd_debug_read_ecs: the first tier's list holds 1 to " + std::to_string(TUPLE_CAP_BIG) + " entries");
  c->rec_chunk = chunk_items; c->rec_small_cap = list_cap;
  if (table_ms) *table_ms = c->rec_table_ms;
  if (items_ms) *items_ms = c->rec_items_ms;
  if (n_second_tier) *n_second_tier = c->rec_second;
  return 0;
}
