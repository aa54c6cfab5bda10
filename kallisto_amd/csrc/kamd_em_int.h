// kamd_em_int.h -- what the EM's translation units share (kamd_em.hip, kamd_em_stream.hip; nobody else includes this): the types that cross a
// unit boundary or sit inside one that does -- all in namespace kamdi, SellCache (which the context owns) and everything inside it included --,
// the constants two units read, and the host functions one unit calls in another.  A kernel lives in ONE unit; where another unit needs it
// launched, the owner has a function for that (pm_refresh_enqueue).
#pragma once
#include "kamd_dev.h"

namespace kamdi {
// Loop control without a control kernel.  Two records, indexed by the parity of the launch: the kernels of a round read
// the record the PREVIOUS round left (iter, final flag, number of transcripts that still changed) and every block derives
// from it -- identically -- what the reference's loop would do next (:202-221); block 0 of k_em_rows publishes that as this
// round's record, k_em_final accumulates the round's change count into it.  Nothing is read and written in the same launch.
struct EmState {
  int iter;         // round index i this record's round ran as (-1: before the first round)
  int chcount;      // transcripts with next > 1e-2 that moved by more than 1 % in that round (:177-179)
  int final_round;  // finalRound: the round read the clamped alpha and was the last one
  int done;
  int rounds;       // i at exit ("ran for i rounds")
  int force_final;  // host request (partitioned EM): the next round is the final round
  int pad[2];
};
struct EmNow { int it, fin, done, rounds; };
__host__ __device__ inline EmNow em_next_round(const EmState& prev, int n_iter, int min_rounds, bool spec) {
  EmNow n; n.it = prev.iter; n.fin = prev.final_round; n.done = prev.done; n.rounds = prev.rounds;
  if (n.done) return n;                                                              // (fin keeps telling how the loop ended)
  if (prev.final_round) { n.done = 1; n.rounds = prev.iter; return n; }              // :207-209 (break: i is not incremented)
  const bool stopEM = !spec && prev.chcount == 0 && prev.iter > min_rounds;          // :202-205
  n.it = prev.iter + 1;
  n.fin = (stopEM || prev.force_final) ? 1 : 0;                                      // :212-221 (clamp applied on read)
  // the loop ran out: round n.it does not run.  With n.fin set it would have been the final round -- the host tells the two apart by
  // rounds == n_iter (kamd_em_local::em_final_round_runs) and clamps the result of round n_iter - 1 itself
  if (n.it >= n_iter) { n.done = 1; n.rounds = n_iter; }
  return n;
}
struct Carver {  // sub-allocations of one device arena, 256-byte aligned
  size_t off = 0;
  size_t take(size_t bytes) { const size_t o = off; off = (off + bytes + 255) & ~(size_t)255; return o; }
};

// ---- streamed form (kernels: kamd_em_stream.hip; the passes both it and the hybrid instantiate: kamd_em_stream.h) ----
constexpr u32 PM_END = 0x80000000u;
constexpr u32 PM_NONE = 0xFFFFFFFFu;
constexpr u32 PM_HEAVY = 0x80000000u;
constexpr u32 PM_LONG = 0x40000000u;      // head word: the crossing segment has more than 64 * PM_HEAD entries before the chunk, at most PM_LOOP_MAX: the chunk re-reads them in a loop
constexpr u32 PM_LOOP_MAX = 32768;
constexpr int PM_BLOCK = 256;         // 4 wavefronts = 4 chunks per block
constexpr int PM_HEAD = 4;            // a crossing segment with <= 64 * PM_HEAD entries before the chunk is re-read by the chunk
constexpr int PM_LDS_SLOTS = 512;     // segment sums staged per wavefront and window
struct PmSide {
  const u32* stream;     // [n_chunks * 64 * K] index | PM_END; the tail padding points at a sentinel whose value is 0; 64 * PM_HEAD
                         // readable entries (any valid index) in front of it
  const u32* seg_base;   // [n_chunks] segment that contains the chunk's first entry
  const u32* head;       // [n_chunks] entries of that segment before the chunk: 0, 1..64*PM_HEAD (re-read), PM_HEAVY (partials)
  const u32* fix_first;  // [n_chunks] heavy crossing segment that ENDS in this chunk: the chunk it started in, else PM_NONE
  const u32* lane_word;  // [n_chunks * 64] per lane of the chunk: segment ends below the lane | ends in the lane << 12 | distance to the
                         // nearest lane at or below it that holds an end (lane + 1: none) << 18 -- what the passes would otherwise
                         // recount from the END flags every round
  double* lp;            // [n_chunks] sum of the chunk's entries up to its first segment end (all of them if there is none)
  double* rp;            // [n_chunks] sum of the entries after the chunk's last segment end
  u32 n_chunks;
};
struct PmArgs {
  PmSide rows, cols;
  const u64* cw;           // [R] count | weight count << 32 of the kept rows
  double* g;               // [R + 1]; g[R] = 0 is the sentinel the column stream's padding points at
  double* alpha0; double* alpha1; double* a0; double* a1;   // [M + 1]; a*[M] = 0 is the row stream's sentinel
  double* ac0; double* ac1;   // [M + 1] a with the final round's clamp (alpha < alpha_limit / 10 -> 0, EMAlgorithm.h:212-221): what the final round reads
  const double* single; const double* eff;   // [M]
  u32 R, M;
  int n_iter, min_rounds;
  EmState* st;             // the two parity-indexed loop-control records (see EmState)
  int* spec_hist;          // partitioned EM: per-round change counts of this rank (the stop rule is applied by the host); else null
};
struct PmPlan {
  PmArgs args{};
  int k = 0;                 // entries per lane
  bool windowed = false;     // some chunk holds more segment ends than a wavefront's LDS slots (or KAMD_EM_WINDOWED=1): the general pass
  u32 n_chunks = 0;
  u32 n_fix[2] = {0, 0};     // heavy crossing segments per direction (0: no fix-up launch)
  const u32* mflag = nullptr; const u64* mpos = nullptr;   // transcript -> m-space
  const u64* roff = nullptr; const u64* coff = nullptr;    // [R + 1] / [M + 1] entry offsets of the rows / columns (the hybrid picks its hot targets by length)
  u32* rs = nullptr; u32* cs = nullptr; u64 nzpad = 0;     // the two entry streams (nzpad entries each)
  const u64* rpos = nullptr;                               // row of the source matrix -> kept row (rows of fewer than two transcripts: unset)
};

// ---- component-local form over the sliced-ELLPACK layout (kamd_em.hip) ----
struct EmSellDev {
  const u32* row_base; const u32* tr_base; const u32* rslice_base; const u32* cslice_base; const u64* rell_base; const u64* cell_base;
  const u32* rdesc; const u32* cdesc; const uint16_t* rell; const uint16_t* cell;
  const u64* cw; const double* single; const double* eff;
  const u32* grec;   // the six bases of group g and of g + 1 as ONE record of 16 words (k_sell_group_rec): a launch fetches it with one scalar load
};

// ---- hybrid: the oversized components beside the component-local form (kamd_em.hip) ----
struct GiDesc { int* hist; int stopped; int pad; };   // this chunk's per-round change counts (null: not wanted); the run stopped in the previous chunk
struct GbSide {
  const uint16_t* stream;   // [n_chunks * GB_CH]; the chunks of a block are consecutive, a block starts on a chunk boundary
  const u32* seg_base;      // [n_chunks] pieces that end in earlier chunks (= id of the chunk's first piece)
  const u32* lane_word;     // [n_chunks * 64] as PmSide::lane_word
  const u32* piece_slot;    // [n_pieces] where a piece's sum goes in `part`
  double* part;             // [n_pieces]
  const u32* slot_base;     // [n_seg + 1] the slots of a segment's pieces: slot_base[s] .. slot_base[s + 1]
  const u32* wg_desc;       // [2 * n_wg] per workgroup: its work items wg_items[first .. end)
  const u32* wg_items;      // [4 * n_items] block, first chunk, end chunk, rotation of the block's load: a workgroup loads the block, then its wavefronts take the chunks
  u32 n_wg, n_chunks, n_pieces, n_seg, n_tgt;
};
struct GbArgs { GbSide rows, cols; const u64* cw; const double* single; const double* eff; u32 R, M; };
struct GbPlan { GbArgs args{}; bool valid = false; };
struct GiantPart {
  PmPlan plan;
  double* G_al[2] = {nullptr, nullptr}; double* G_a[2] = {nullptr, nullptr};   // the ping-pong state of the chunks (chunk k: [k & 1] -> [(k + 1) & 1])
  double* S_al[2] = {nullptr, nullptr}; double* S_a[2] = {nullptr, nullptr};   // what the rounds inside a chunk alternate between
  double* ac = nullptr;
  GiDesc* desc = nullptr;
  hipStream_t stream = nullptr; hipEvent_t ev = nullptr;
  hipGraph_t graph[2] = {nullptr, nullptr}; hipGraphExec_t gexec[2] = {nullptr, nullptr};
  bool use_graph = true;
  u64 nnz = 0, rows = 0;
  GbPlan gb;   // the same rounds in 2-D blocks with the gathers out of LDS (gb.valid), three launches per round instead of k_gi_rows / k_gi_cols
  void drop_graphs() {
    for (int i = 0; i < 2; i++) {
      if (gexec[i]) (void)hipGraphExecDestroy(gexec[i]);
      if (graph[i]) (void)hipGraphDestroy(graph[i]);
      gexec[i] = nullptr; graph[i] = nullptr;
    }
  }
};
struct SellCache {
  bool valid = false;
  const u64* d_ec_off = nullptr; const u32* d_ec_ids = nullptr; u64 n_ecs = 0, nnz = 0, T = 0, generation = 0;
  int split_len = 0, group_div = 0, small_nnz = 0;
  bool host_maps = false;   // P.tr_id / P.single_all were read back (the host-side scatter of several ranks needs them)
  kamd_em_sell::Plan P;      // host part (tr_id, single_all, bases)
  EmSellDev dev{};           // device part, in ctx->ems_plan
  u32* row_final = nullptr; u32* mslot = nullptr; double* single_all = nullptr; double* d_eff = nullptr;   // in ctx->ems_maps
  bool hybrid = false;       // G holds the streamed plan of the components beyond a workgroup's LDS; P / dev the others
  GiantPart G;
  // what a cached hybrid plan needs to take new counts (a bootstrap replicate): the split of the rows into the two sub-matrices (arrays in ctx->hy_sub)
  struct HyKeep {
    const u32* flag_s = nullptr; const u32* flag_g = nullptr; const u64* rpos_s = nullptr; const u64* rpos_g = nullptr;
    const u64* off_s = nullptr; const u64* off_g = nullptr; const u32* ids_s = nullptr; const u32* ids_g = nullptr;
    u32* cnt_s = nullptr; u32* cnt_g = nullptr; u32* wc_s = nullptr; u32* wc_g = nullptr;
    u64 n_s = 0, n_g = 0; bool no_groups = false;
  } hy;
  int giant_nnz_t = 0, blocked_t = 0, hybrid_t = 0;   // tuning the cached plan was built under
  ~SellCache() { G.drop_graphs(); }
};

// kamd_em_stream.hip
// returns 0 = plan built (the rounds can be enqueued with pm_enqueue_round), 1 = not applicable (the caller uses the CSR
// form), < 0 = error.  Needs col_cnt / em_coloff / em_single / em_eff of the caller (k_em_prepare + scan) and a zeroed col_fill.
int em_streamed_setup(kamd_ctx* c, const u64* ec_off, const u32* ec_ids, const u32* counts, const u32* wcounts, u64 n_ecs, u64 T,
                      const u32* col_cnt, u32* col_fill, PmPlan* P, DBuf* arena_a = nullptr, DBuf* arena_b = nullptr);
void pm_enqueue_round(const PmPlan& P, hipStream_t s, int parity);
// k_pm_minit on the context stream for a plan that is kept: the singleton counts and effective lengths in c->em_single / c->em_eff into
// m-space, the vectors back at alpha = 1 / T; the layout stays
void pm_refresh_enqueue(kamd_ctx* c, const PmPlan& P, u64 T);
}  // namespace kamdi
