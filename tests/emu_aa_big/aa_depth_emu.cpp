// tests/emu_aa_big/aa_depth_emu.cpp -- TEST INFRASTRUCTURE: how deep the class lists of the translated search (kallisto_amd/csrc/kamd_aa.h) get,
// read by read on the CPU, beside tests/emu_aa/aa_emu.cpp, which gives the reads' outcomes and sets.  Never linked into libkallisto_amd.so.
#include "../../include/kallisto_amd.h"
#include "../../kallisto_amd/csrc/kamd_aa.h"

#include <vector>

extern "C" {
// Per read: list_len[i] = the longest class list among its six frames -- how deep into its lane's scratch slab the kernel goes for it;
// win_sets[i] = the distinct index sets of the winning frame (0: not aligned; 1: the kernel counts the read in the dense vector; more: it
// writes a tuple record).  Returns the longest list met, -1 if a list overflows max_len + 2 entries.
int64_t aa_emu_list_depth(const kamd_index_view* v, const uint32_t* words, const uint16_t* lens, uint64_t n, int32_t max_len, uint32_t* list_len,
                          uint32_t* win_sets) {
  using namespace kamd;
  const int sw = (max_len + 15) / 16 + 1, rec = sw + (max_len + 31) / 32 + 1;
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
  std::vector<uint64_t> lists((size_t)cap_l * 6);
  std::vector<uint32_t> frame((size_t)rec);
  int64_t longest = 0;
  for (uint64_t i = 0; i < n; i++) {
    const uint32_t* src = words + i * rec;
    const int l = lens[i];
    AaClassList cl[6];
    uint32_t card[6], taint = 0;
    int deepest = 0;
    for (int f = 0; f < 6; f++) {
      for (int w = 0; w < rec; w++) frame[w] = aa_frame_word(src, src + sw, l, f, w, sw);
      const ReadView r{frame.data(), frame.data() + sw, aa_translated_len(l, f)};
      cl[f] = AaClassList{lists.data() + (size_t)f * cap_l, 1, cap_l, 0, false};
      aa_match_frame(t, ax, r, aa_frame_len(l, f), v->k, cl[f], nullptr);
      if (cl[f].overflow) return -1;
      if (cl[f].n > deepest) deepest = cl[f].n;
      const AaFrameSet fs = aa_frame_set(st, offlist.data(), cl[f]);
      card[f] = fs.taint ? 0u : fs.card;
      if (fs.taint) taint |= 1u << f;
    }
    const AaDecision d = aa_read_rule(card, taint);
    list_len[i] = (uint32_t)deepest;
    win_sets[i] = d.outcome == AA_ALIGNED ? (uint32_t)aa_classlist_to_sets(cl[d.winner]) : 0u;
    if (deepest > longest) longest = deepest;
  }
  return longest;
}
}
