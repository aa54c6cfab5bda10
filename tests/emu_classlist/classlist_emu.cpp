// tests/emu_classlist/classlist_emu.cpp -- TEST INFRASTRUCTURE: what tests/emu/emu.cpp does not lay open.  emu_class_list: the class list of ONE item
// as kernel A's stepper builds it (emu_tuples' loop, restated here, reports the mapped sets only).  emu_ec_state_opts: emu_ec_state with --no-jump,
// --union and set lists of up to 1024 entries.  Both take the index view of an index loaded through tests/emu (tests/emu_binding.EmuIndex).
// Never linked into libkallisto_amd.so.
#include "../../include/kallisto_amd.h"
#include "../../kallisto_amd/csrc/kamd_core.h"

#include <cstring>
#include <vector>

// the k-mer table(s) of the host view as the per-item logic sees them (mirrors make_table of kamd_dev.h, as tests/emu/emu.cpp does)
static kamd::Table emu_table(const kamd_index_view* v, bool partial, bool no_jump) {
  kamd::Table t{v->table, v->n_buckets};
  t.layout = (uint8_t)v->table_layout; t.q = (uint8_t)v->tag_q; t.dsh = (uint8_t)v->tag_dsh; t.tagw = (uint8_t)v->tag_w;
  t.dslots = v->dtable; t.n_dbuckets = v->n_dbuckets; t.dummy_uec = v->dummy_uec; t.dummy_slot = v->dummy_slot;
  t.dummy_strand = v->dummy_strand != 0; t.partial = partial; t.no_jump = no_jump;
  return t;
}

// The class list of ONE item (entries: class | mate flags in bits 30 / 31): the distinct classes of the first pass (flags bit 3 clear) or the
// append-only list of the second pass (bit 3 set: duplicates stay unless they are neighbours).  flags as emu_tuples' use_stepper: bit 1 --no-jump,
// bit 2 the unitig text in front of the table (kernel A v3), bit 3 append.  Returns the number of entries, -2 beyond cap.
extern "C" int64_t emu_class_list(const kamd_index_view* v, const uint32_t* words, const uint16_t* lens, uint64_t item, int paired,
                                  int32_t max_len, int flags, uint32_t* out, uint64_t cap) {
  using namespace kamd;
  const uint64_t sw = (uint64_t)(max_len + 15) / 16 + 1, rec = kamd_packed_record_words(max_len);
  const Table t = emu_table(v, !paired, (flags & 2) != 0);
  const bool use_text = (flags & 4) != 0;
  UecList ul{out, (int)cap, 0, false};
  ul.append = (flags & 8) != 0;
  MateFirst mf[2] = {{0, 0, -1, false}, {0, 0, -1, false}};
  for (int mate = 0; mate < (paired ? 2 : 1); mate++) {
    const uint64_t r = paired ? 2 * item + mate : item;
    ReadView rv{words + r * rec, words + r * rec + sw, lens[r]};
    rv.has_n = (rv.seq[sw - 1] & REC_FLAG_HAS_N) != 0;   // the packers' has-N flag word decides whether the mask plane is consulted
    MatchState st; match_init(st, rv, v->k);
    while (st.phase != PH_DONE) {
      bool fc; const uint64_t canon = window_canon(rv, st.w, v->k, &fc);
      Probe p; p.found = false;
      if (use_text && text_applies(st)) {
        if (text_canon(v->utext, text_pos_of(st), v->k) == canon) {
          p.found = true; p.strand = st.um_strand; p.uec = st.um_uec; p.dist = 0; p.slot = 0; p.gpos = 0;
        } else { st.text_tried = true; continue; }
      } else if (use_text) {   // as kernel A v3: one bucket per step, a continue flag costs another step
        const Table pt = phase_table(t, st.phase);
        const uint32_t h = kmer_hash32(canon);
        const uint64_t b = bucket_of_hash(h, pt.n_buckets) + st.disp;
        if (pt.layout == LAYOUT_COMPACT) {
          if (match_bucket_compact(load_bucket(pt.slots, b), pt, compact_tag(pt, canon, h, st.disp), fc, b, p) == BUCKET_CONTINUE &&
              st.disp < compact_max_disp(pt)) { ++st.disp; continue; }
        } else if (match_bucket(load_bucket(pt.slots, b), canon, fc, b, p) == BUCKET_CONTINUE) { ++st.disp; continue; }
      } else {
        p = probe_table(phase_table(t, st.phase), canon, fc, nullptr);
      }
      if (t.n_dbuckets) match_feed<true>(st, rv, v->k, p, ul, mate, mf[mate], t); else match_feed<false>(st, rv, v->k, p, ul, mate, mf[mate], t);
    }
  }
  return ul.overflow ? -2 : (int64_t)ul.n;
}

// The straight-line matcher's EC state: dense[n_ecs] += single-set items, tuple records [1, m, e0..] appended to stream (capacity cap words).
// mode bit 0: --no-jump, bit 1: --union (a record's sets carry the mate flags EC_MATE1 / EC_MATE2, a single set is counted in `dense` without
// them).  The items are item_ids[0 .. n_items) of the packed reads (nullptr: all, in order).
extern "C" int64_t emu_ec_state_opts(const kamd_index_view* v, const uint32_t* words, const uint16_t* lens, const uint64_t* item_ids, uint64_t n_items,
                                     int paired, int32_t max_len, int mode, uint32_t* dense, uint32_t* stream, uint64_t cap, uint64_t* rec_off,
                                     uint64_t* n_recs) {
  using namespace kamd;
  const bool no_jump = (mode & 1) != 0, do_union = (mode & 2) != 0;
  const uint64_t sw = (uint64_t)(max_len + 15) / 16 + 1, rec = kamd_packed_record_words(max_len);
  const Table t = emu_table(v, !paired && !do_union, no_jump);
  std::vector<uint8_t> nonempty(v->n_ecs);
  for (uint64_t e = 0; e < v->n_ecs; e++) nonempty[e] = v->ec_off[e + 1] > v->ec_off[e];
  uint64_t o = 0, nr = 0;
  uint32_t ecbuf[1024];
  for (uint64_t q = 0; q < n_items; q++) {
    const uint64_t i = item_ids ? item_ids[q] : q;
    EcList ecs{ecbuf, 1024, 0, false};
    MateInfo m[2]; memset(m, 0, sizeof m);
    for (int mate = 0; mate < (paired ? 2 : 1); mate++) {
      const uint64_t r = paired ? 2 * i + mate : i;
      ReadView rv{words + r * rec, words + r * rec + sw, lens[r]};
      match_mate(t, v->uec_ec, nonempty.data(), rv, v->k, ecs, m[mate], do_union ? (mate ? EC_MATE2 : EC_MATE1) : 0u);
    }
    if (ecs.overflow) return -1;
    if (!pair_is_mapped(m[0], m[1])) continue;
    if (ecs.n == 1) { dense[ecs.e[0] & EC_ID_MASK]++; continue; }
    if (o + ecs.n + 2 > cap) return -2;
    rec_off[nr++] = o;
    stream[o++] = 1; stream[o++] = (uint32_t)ecs.n;
    for (int j = 0; j < ecs.n; j++) stream[o++] = ecs.e[j];
  }
  *n_recs = nr;
  return (int64_t)o;
}
