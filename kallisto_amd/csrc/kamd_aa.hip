// kamd_aa.hip -- translated search (`bus --aa`): nucleotide reads against an index of amino-acid sequences, both in the comma-free code.
//   k_aa_translate   packed reads -> six packed frame records per read (kamd_aa.h: aa_frame_word); one thread owns one output word
//   k_aa_match       the six frames of a read in six adjacent lanes of an eight-lane group: match (aa_match_frame), the frame's set under
//                    dfk_onlist (aa_frame_set), the read rule across the group's lanes (aa_read_rule); the winning lane hands the read to the
//                    context's EC state -- a single set to the dense counts, several as a tuple record [1, m, e0..] that absorb_tuples takes like
//                    the records of k_pseudoalign_overflow.  A winner has no off-list member, so all its sets are on-list and the plain
//                    intersection kamd_ec_finalize resolves equals the one the frame rule counted.
// The per-item semantics live in kamd_aa.h (shared with the CPU emulation of tests/emu_aa).
#include "kamd_dev.h"
#include "kamd_aa.h"

namespace {

constexpr int AA_GROUP = 8;                 // lanes per read: frames 0..5, two idle lanes; a wavefront holds eight reads
constexpr int AA_LIST_CAP = 1024;           // classes kept per frame (a frame of l bases has at most l - k + 1 windows and the D-list's dummy hit)
constexpr u64 AA_CHUNK = 262144;            // reads per launch of kamd_pseudoalign_aa (bounds the frame records and the record stream)
constexpr size_t AA_SCRATCH_MAX = 512u << 20;

struct AaCounters { u64 rejected_offlist, all_empty, clashes, winner[kamd::AA_FRAMES], list_overflow; };

// one byte per index set: the set has a member that is not on-list
__global__ __launch_bounds__(BLOCK) void k_aa_offlist(const u64* __restrict__ ec_off, const u32* __restrict__ ec_ids, const u32* __restrict__ onlist_bits,
                                                      u64 n_ecs, uint8_t* out) {
  const u64 e = (u64)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n_ecs) return;
  uint8_t off = 0;
  for (u64 j = ec_off[e]; j < ec_off[e + 1] && !off; j++) off = onlisted(onlist_bits, ec_ids[j]) ? 0 : 1;
  out[e] = off;
}

// thread t owns word t % rec_words of frame record t / rec_words (= 6 * read + frame): consecutive threads store consecutive words
__global__ __launch_bounds__(BLOCK) void k_aa_translate(const u32* __restrict__ words, const uint16_t* __restrict__ lens, u64 n_reads, int seq_words,
                                                        int rec_words, int max_len, u32* __restrict__ out_words, uint16_t* __restrict__ out_len) {
  const u64 t = (u64)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_reads * (u64)kamd::AA_FRAMES * (u64)rec_words) return;
  const u64 fr = t / (u64)rec_words;
  const int widx = (int)(t - fr * (u64)rec_words);
  const u64 read = fr / kamd::AA_FRAMES;
  const int f = (int)(fr - read * kamd::AA_FRAMES);
  const u32* src = words + read * (u64)rec_words;
  const int l = min((int)lens[read], max_len);   // (a record holds max_len bases)
  out_words[t] = kamd::aa_frame_word(src, src + seq_words, l, f, widx, seq_words);
  if (widx == 0) out_len[fr] = (uint16_t)kamd::aa_translated_len(l, f);
}

struct AaOut { u32* dense; u32* stream; u64* rec_off; DevState* st; AaCounters* ctr; };

// Persistent wavefronts: wavefront w takes the groups of eight reads w, w + W, ...; lane = 8 * (read of the group) + frame.  The class list of a lane lies
// in global scratch, entry j of lane l at [j * 64 + l] of the wavefront's slab (lanes that insert at the same depth touch one line).  A lane whose frame
// has no window (a short frame, the two idle lanes) skips the match and joins the others at the shuffles below: nobody waits for it.
__global__ __launch_bounds__(BLOCK) void k_aa_match(DevIndex ix, const u32* __restrict__ frames, const uint16_t* __restrict__ flen,
                                                    const uint16_t* __restrict__ rlen, u64 n_reads, int seq_words, int rec_words, u64* scratch, int cap,
                                                    const uint8_t* __restrict__ ec_offlist, AaOut out) {
  const int lane = lane_id();
  const u64 wave = (u64)blockIdx.x * (BLOCK / 64) + (threadIdx.x >> 6), n_waves = (u64)gridDim.x * (BLOCK / 64);
  const int f = lane & (AA_GROUP - 1), base = lane & ~(AA_GROUP - 1);
  const kamd::Table t = make_table(ix, false);
  const kamd::AaIndex ax{ix.uec_ec, ix.ec_nonempty, ix.slot_block, ix.blk_unitig};
  const kamd::SetTables st{(const uint64_t*)ix.ec_off, ix.ec_ids};
  u64* my = scratch + wave * 64 * (u64)cap + lane;
  u32 s_single = 0, s_multi = 0, s_proc = 0, s_rej = 0, s_empty = 0, s_clash = 0, s_won = 0, s_ovf = 0;
  const u64 n_groups = (n_reads + (64 / AA_GROUP) - 1) / (64 / AA_GROUP);
  for (u64 g = wave; g < n_groups; g += n_waves) {
    const u64 read = g * (64 / AA_GROUP) + (u64)(lane >> 3);
    const bool have = read < n_reads;
    const bool active = have && f < kamd::AA_FRAMES;
    kamd::AaClassList cl{(uint64_t*)my, 64, cap, 0, false};
    u32 card = 0; bool taint = false;
    if (active) {
      const u64 fr = read * kamd::AA_FRAMES + (u64)f;
      const u32* rec = frames + fr * (u64)rec_words;
      const kamd::ReadView r{rec, rec + seq_words, (int)flen[fr]};
      if (r.len >= ix.k) {
        kamd::aa_match_frame(t, ax, r, kamd::aa_frame_len((int)rlen[read], f), ix.k, cl, nullptr);
        if (cl.overflow) ++s_ovf;
        else { const kamd::AaFrameSet fs = kamd::aa_frame_set(st, ec_offlist, cl); card = fs.card; taint = fs.taint; }
      }
    }
    // the read rule, decided in every lane of the group from the six lanes' results
    u32 cards[kamd::AA_FRAMES];
#pragma unroll
    for (int j = 0; j < kamd::AA_FRAMES; j++) cards[j] = (u32)__shfl((int)card, base + j, 64);
    const u32 tmask = (u32)((__ballot(taint) >> base) & 0x3Full);
    const kamd::AaDecision d = kamd::aa_read_rule(cards, tmask);
    if (have && f == 0) {
      ++s_proc;
      if (d.outcome == kamd::AA_REJECT_OFFLIST) ++s_rej;
      else if (d.outcome == kamd::AA_REJECT_EMPTY) ++s_empty;
      else s_clash += d.clashes;
    }
    if (active && d.outcome == kamd::AA_ALIGNED && d.winner == f) {
      ++s_won;
      const int m = kamd::aa_classlist_to_sets(cl);
      if (m == 1) { atomicAdd(&out.dense[(u32)cl.e[0]], 1u); ++s_single; }
      else {
        const u64 off = atomicAdd(&out.st->stream_words, (u64)m + 2);
        u32* w = out.stream + off;
        w[0] = 1u; w[1] = (u32)m;
        for (int j = 0; j < m; j++) w[2 + j] = (u32)cl.e[j * cl.stride];
        out.rec_off[read] = off;
        ++s_multi;
      }
    }
  }
  // one set of atomics per wavefront
  const u64 w_single = wave_sum64(s_single), w_multi = wave_sum64(s_multi), w_proc = wave_sum64(s_proc), w_rej = wave_sum64(s_rej),
            w_empty = wave_sum64(s_empty), w_clash = wave_sum64(s_clash), w_ovf = wave_sum64(s_ovf);
  u64 w_won[kamd::AA_FRAMES];
#pragma unroll
  for (int j = 0; j < kamd::AA_FRAMES; j++) w_won[j] = wave_sum64(f == j ? (u64)s_won : 0ULL);
  if (lane == 0) {
    if (w_single) atomicAdd(&out.st->st_single, w_single);
    if (w_multi) atomicAdd(&out.st->st_multi, w_multi);
    if (w_proc) atomicAdd(&out.st->st_processed, w_proc);
    if (w_rej) atomicAdd(&out.ctr->rejected_offlist, w_rej);
    if (w_empty) atomicAdd(&out.ctr->all_empty, w_empty);
    if (w_clash) atomicAdd(&out.ctr->clashes, w_clash);
    if (w_ovf) atomicAdd(&out.ctr->list_overflow, w_ovf);
#pragma unroll
    for (int j = 0; j < kamd::AA_FRAMES; j++) if (w_won[j]) atomicAdd(&out.ctr->winner[j], w_won[j]);
  }
}

int aa_check_batch(kamd_ctx* c, const void* w, const void* l, int32_t max_len, const char* who) {
  if (!c) return kamd::fail(-1, std::string(who) + ": null context");
  if (!w || !l) return kamd::fail(-1, std::string(who) + ": null argument");
  if (max_len <= 0 || max_len > 65535) return kamd::fail(-1, std::string(who) + ": max_len must be in [1, 65535]");
  return 0;
}
int aa_launch_translate(kamd_ctx* c, const u32* d_words, const uint16_t* d_len, u64 n, int32_t max_len, u32* out_words, uint16_t* out_len) {
  const int seq_words = (max_len + 15) / 16 + 1, rec_words = (int)kamd_packed_record_words(max_len);
  const u64 total = n * (u64)kamd::AA_FRAMES * (u64)rec_words;
  if (grid_for(total, BLOCK) == 0 || total / BLOCK >= 0x7FFFFFFFULL) return kamd::fail(-1, "kamd_cfc_frames: batch too large for one launch");
  hipLaunchKernelGGL(k_aa_translate, dim3(grid_for(total, BLOCK)), dim3(BLOCK), 0, c->stream, d_words, d_len, n, seq_words, rec_words, (int)max_len, out_words, out_len);
  HIPC(hipGetLastError());
  return 0;
}

}  // namespace

extern "C" int kamd_cfc_frames(kamd_ctx* c, const uint32_t* d_words, const uint16_t* d_len, uint64_t n_reads, int32_t max_len, uint32_t* d_out_words,
                               uint16_t* d_out_len) {
  if (int rc = aa_check_batch(c, d_words, d_len, max_len, "kamd_cfc_frames")) return rc;
  if (!d_out_words || !d_out_len) return kamd::fail(-1, "kamd_cfc_frames: null output");
  if (n_reads == 0) return 0;
  HIPC(hipSetDevice(c->device));
  for (u64 first = 0; first < n_reads; first += AA_CHUNK) {
    const u64 n = std::min(AA_CHUNK, n_reads - first);
    const u64 rec_words = kamd_packed_record_words(max_len);
    if (int rc = aa_launch_translate(c, d_words + first * rec_words, d_len + first, n, max_len, d_out_words + first * kamd::AA_FRAMES * rec_words,
                                     d_out_len + first * kamd::AA_FRAMES)) return rc;
  }
  return 0;
}

extern "C" int kamd_pseudoalign_aa(kamd_ctx* c, const uint32_t* d_words, const uint16_t* d_len, uint64_t n_reads, int32_t max_len) {
  if (int rc = aa_check_batch(c, d_words, d_len, max_len, "kamd_pseudoalign_aa")) return rc;
  if (!c->has_index) return kamd::fail(-1, "kamd_pseudoalign_aa: no index uploaded");
  if (c->track_order) return kamd::fail(-5, "kamd_pseudoalign_aa: not with kamd_ec_track_order");
  if (c->ix.n_shades) return kamd::fail(-5, "kamd_pseudoalign_aa: the translated search is not defined for an index with shades");
  if (n_reads == 0) return 0;
  HIPC(hipSetDevice(c->device));
  if (c->ov_side_pending) { HIPC(hipStreamSynchronize(c->ov_stream)); c->ov_side_pending = false; }
  for (hipEvent_t& e : c->aa_ev) if (!e) HIPC(hipEventCreate(&e));
  DevIndex ix = c->ix;
  ix.no_jump = 0; ix.union_mode = 0; ix.comprehensive = 0;   // (what an earlier kamd_pseudoalign left there; neither option exists with --aa)
  if (!c->aa_ready) {
    if (int rc = c->aa_offlist.ensure(std::max<u64>(c->n_ecs, 1), 0, c->stream)) return rc;
    hipLaunchKernelGGL(k_aa_offlist, dim3(grid_for(std::max<u64>(c->n_ecs, 1), BLOCK)), dim3(BLOCK), 0, c->stream, ix.ec_off, ix.ec_ids, ix.onlist_bits, c->n_ecs,
                       c->aa_offlist.as<uint8_t>());
    HIPC(hipGetLastError());
    c->aa_ready = true;
  }
  const int seq_words = (max_len + 15) / 16 + 1, rec_words = (int)kamd_packed_record_words(max_len);
  const int cap = std::min(AA_LIST_CAP, std::max(1, max_len - ix.k + 2));
  const u64 chunk_max = std::min<u64>(AA_CHUNK, n_reads);
  if (int rc = c->aa_frames.ensure((chunk_max * kamd::AA_FRAMES * (u64)rec_words + 4) * sizeof(u32), 0, c->stream)) return rc;
  if (int rc = c->aa_flen.ensure(chunk_max * kamd::AA_FRAMES * sizeof(uint16_t), 0, c->stream)) return rc;
  if (int rc = c->aa_ctr.ensure(sizeof(AaCounters), 0, c->stream)) return rc;
  if (int rc = c->stream_buf.ensure(chunk_max * (u64)(cap + 2) * sizeof(u32), 0, c->stream)) return rc;
  if (int rc = c->rec_off.ensure(chunk_max * sizeof(u64), 0, c->stream)) return rc;
  // as many wavefronts as are worth keeping resident (sixteen per CU), fewer when the batch is small or their class lists would not fit
  const u64 groups = (chunk_max + 7) / 8;
  u64 blocks = std::min<u64>((groups + BLOCK / 64 - 1) / (BLOCK / 64), (u64)std::max(1, c->n_cus) * 4);
  blocks = std::max<u64>(1, std::min<u64>(blocks, AA_SCRATCH_MAX / ((size_t)BLOCK * cap * sizeof(u64))));
  if (int rc = c->aa_scratch.ensure(blocks * BLOCK * (u64)cap * sizeof(u64), 0, c->stream)) return rc;
  HIPC(hipMemsetAsync(c->aa_ctr.p, 0, sizeof(AaCounters), c->stream));
  float tr_ms = 0.f, ma_ms = 0.f;
  uint32_t launches = 0;
  for (u64 first = 0; first < n_reads; first += AA_CHUNK) {
    const u64 n = std::min(AA_CHUNK, n_reads - first);
    const u32* w = d_words + first * (u64)rec_words;
    const uint16_t* l = d_len + first;
    c->host_state.stream_words = 0; c->host_state.n_recs = n;
    if (int rc = push_state(c)) return rc;
    HIPC(hipMemsetAsync(c->rec_off.p, 0xFF, n * sizeof(u64), c->stream));   // ~0 = the read has no tuple record
    HIPC(hipEventRecord(c->aa_ev[0], c->stream));
    if (int rc = aa_launch_translate(c, w, l, n, max_len, c->aa_frames.as<u32>(), c->aa_flen.as<uint16_t>())) return rc;
    HIPC(hipEventRecord(c->aa_ev[1], c->stream));
    const AaOut out{c->dense.as<u32>(), c->stream_buf.as<u32>(), c->rec_off.as<u64>(), (DevState*)c->state.p, c->aa_ctr.as<AaCounters>()};
    hipLaunchKernelGGL(k_aa_match, dim3((unsigned)blocks), dim3(BLOCK), 0, c->stream, ix, (const u32*)c->aa_frames.as<u32>(), (const uint16_t*)c->aa_flen.as<uint16_t>(), l, n,
                       seq_words, rec_words, c->aa_scratch.as<u64>(), cap, (const uint8_t*)c->aa_offlist.as<uint8_t>(), out);
    HIPC(hipGetLastError());
    ++launches;
    HIPC(hipEventRecord(c->aa_ev[2], c->stream));
    if (int rc = sync_state(c)) return rc;
    { float a = 0.f, b = 0.f; HIPC(hipEventElapsedTime(&a, c->aa_ev[0], c->aa_ev[1])); HIPC(hipEventElapsedTime(&b, c->aa_ev[1], c->aa_ev[2])); tr_ms += a; ma_ms += b; }
    if (int rc = absorb_tuples(c, c->stream_buf.as<u32>(), c->rec_off.as<u64>(), n, c->host_state.stream_words, c->recs_total,
                               c->host_state.st_multi - c->multi_before)) return rc;
    c->multi_before = c->host_state.st_multi;
    c->recs_total += n;
    c->finalized = false;
  }
  AaCounters ctr{};
  HIPC(hipMemcpyAsync(&ctr, c->aa_ctr.p, sizeof ctr, hipMemcpyDeviceToHost, c->stream));
  HIPC(hipStreamSynchronize(c->stream));
  if (ctr.list_overflow)
    return kamd::fail(-4, "kamd_pseudoalign_aa: a frame's hits carry more than " + std::to_string(cap) + " classes; the batch is not counted in full (kamd_ec_reset and shorter reads)");
  kamd_aa_stats& s = c->aa_stats;
  s.n_processed += n_reads; s.n_rejected_offlist += ctr.rejected_offlist; s.n_all_empty += ctr.all_empty; s.n_frame_clashes += ctr.clashes;
  for (int j = 0; j < kamd::AA_FRAMES; j++) s.n_winner[j] += ctr.winner[j];
  s.last_translate_ms = tr_ms; s.last_match_ms = ma_ms;
  s.last_chunks = launches; s.last_match_blocks = (uint32_t)blocks; s.last_list_cap = (uint32_t)cap;
  return 0;
}

extern "C" int kamd_aa_stats_get(kamd_ctx* c, kamd_aa_stats* out) {
  if (!c || !out) return kamd::fail(-1, "kamd_aa_stats_get: null argument");
  *out = c->aa_stats;
  return 0;
}
