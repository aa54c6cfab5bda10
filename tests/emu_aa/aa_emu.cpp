// tests/emu_aa/aa_emu.cpp -- TEST INFRASTRUCTURE: drives the per-item logic of the translated search (kallisto_amd/csrc/kamd_aa.h) on
// the CPU, read by read, the way the kernels of kamd_aa.hip do lane by lane.  Never linked into libkallisto_amd.so.
#include "../../include/kallisto_amd.h"
#include "../../kallisto_amd/csrc/kamd_aa.h"

#include <cstring>
#include <vector>

extern "C" {
void aa_emu_codon_table(uint8_t* out64) { for (uint32_t c = 0; c < 64; c++) out64[c] = (uint8_t)kamd::cfc_of_codon(c); }

// six frame records per read (record 6 * i + f, the layout of the input records) and their translated lengths
void aa_emu_frames(const uint32_t* words, const uint16_t* lens, uint64_t n, int32_t max_len, uint32_t* out_words, uint16_t* out_len) {
  const int sw = (max_len + 15) / 16 + 1, rec = (int)kamd_packed_record_words(max_len);
  for (uint64_t i = 0; i < n; i++)
    for (int f = 0; f < kamd::AA_FRAMES; f++) {
      const uint32_t* src = words + i * rec;
      for (int w = 0; w < rec; w++) out_words[(i * 6 + f) * rec + w] = kamd::aa_frame_word(src, src + sw, lens[i], f, w, sw);
      out_len[i * 6 + f] = (uint16_t)kamd::aa_translated_len(lens[i], f);
    }
}

// Per read: outcome[i] = winning frame 0..5, -1 = rejected for an off-list member, -2 = all frames empty; clashes[i]; the winner's
// transcript set in out_ids[out_off[i] .. out_off[i+1]).  diag (optional, 3 words): reads where the early return of the frame
// intersection left an off-list set unvisited; reads with a frame whose class list differs when the jump clamp takes the
// translated length; reads rejected by step 1 of the read rule that would be aligned without it.
int64_t aa_emu_pseudoalign(const kamd_index_view* v, const uint32_t* words, const uint16_t* lens, uint64_t n, int32_t max_len,
                           int32_t* outcome, uint32_t* clashes, uint64_t* out_off, uint32_t* out_ids, uint64_t cap, uint64_t* diag) {
  using namespace kamd;
  const int sw = (max_len + 15) / 16 + 1, rec = (int)kamd_packed_record_words(max_len);
  Table t{v->table, v->n_buckets};
  t.layout = (uint8_t)v->table_layout; t.q = (uint8_t)v->tag_q; t.dsh = (uint8_t)v->tag_dsh; t.tagw = (uint8_t)v->tag_w;
  t.dslots = v->dtable; t.n_dbuckets = v->n_dbuckets; t.dummy_uec = v->dummy_uec; t.dummy_slot = v->dummy_slot;
  t.dummy_strand = v->dummy_strand != 0; t.partial = false; t.no_jump = false;
  std::vector<uint8_t> nonempty(v->n_ecs + 1), offlist(v->n_ecs + 1);
  for (uint64_t e = 0; e < v->n_ecs; e++) {
    nonempty[e] = v->ec_off[e + 1] > v->ec_off[e];
    for (uint64_t j = v->ec_off[e]; j < v->ec_off[e + 1]; j++) {
      const uint32_t x = v->ec_ids[j];
      if (!((v->onlist_bits[x >> 5] >> (x & 31)) & 1u)) offlist[e] = 1;
    }
  }
  const AaIndex ax{v->uec_ec, nonempty.data(), v->slot_block, v->blk_unitig};
  const SetTables st{v->ec_off, v->ec_ids};
  const int cap_l = max_len + 2;
  std::vector<uint64_t> lists((size_t)cap_l * 6), alt((size_t)cap_l);
  std::vector<uint32_t> frame((size_t)rec);
  if (diag) diag[0] = diag[1] = diag[2] = 0;
  uint64_t o = 0;
  for (uint64_t i = 0; i < n; i++) {
    out_off[i] = o;
    const uint32_t* src = words + i * rec;
    const int l = lens[i];
    AaClassList cl[6];
    uint32_t card[6], card_off[6], taint = 0;
    bool early = false, differs = false;
    for (int f = 0; f < 6; f++) {
      for (int w = 0; w < rec; w++) frame[w] = aa_frame_word(src, src + sw, l, f, w, sw);
      const ReadView r{frame.data(), frame.data() + sw, aa_translated_len(l, f)};
      cl[f] = AaClassList{lists.data() + (size_t)f * cap_l, 1, cap_l, 0, false};
      aa_match_frame(t, ax, r, aa_frame_len(l, f), v->k, cl[f], nullptr);
      if (cl[f].overflow) return -1;
      const AaFrameSet fs = aa_frame_set(st, offlist.data(), cl[f], diag ? v->onlist_bits : nullptr);
      card[f] = fs.taint ? 0u : fs.card; card_off[f] = fs.card;
      if (fs.taint) taint |= 1u << f;
      early = early || fs.early_taint;
      if (diag) {
        AaClassList c2{alt.data(), 1, cap_l, 0, false};
        aa_match_frame(t, ax, r, r.len, v->k, c2, nullptr);
        bool same = c2.n == cl[f].n;
        for (int j = 0; same && j < c2.n; j++) same = c2.e[j] == cl[f].e[j];
        differs = differs || !same;
      }
    }
    const AaDecision d = aa_read_rule(card, taint);
    clashes[i] = d.clashes;
    outcome[i] = d.outcome == AA_ALIGNED ? d.winner : (d.outcome == AA_REJECT_OFFLIST ? -1 : -2);
    if (diag) {
      diag[0] += early; diag[1] += differs;
      if (d.outcome == AA_REJECT_OFFLIST && aa_read_rule(card_off, 0u).outcome == AA_ALIGNED) ++diag[2];
    }
    if (d.outcome == AA_ALIGNED) {
      bool full = false;
      aa_for_each_common(st, cl[d.winner], cl[d.winner].n, [&](uint32_t x) { if (o < cap) out_ids[o++] = x; else full = true; });
      if (full) return -2;
    }
  }
  out_off[n] = o;
  return (int64_t)o;
}
}
