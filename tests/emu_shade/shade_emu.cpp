// tests/emu_shade/shade_emu.cpp -- TEST INFRASTRUCTURE: the per-item logic of kallisto_amd/csrc/kamd_core.h on an index with shades, driven on
// the CPU the way the straight-line kernels of kamd_match.hip drive it (k_explicit_write for the class, k_fld for the fragment length), so that
// the class rule can be checked against the reference's goldens on a box without a GPU.  Never linked into libkallisto_amd.so.
#include "../../include/kallisto_amd.h"
#include "../../kallisto_amd/csrc/kamd_core.h"

#include <algorithm>
#include <cstring>
#include <vector>

// Per item: its class after the on-list mask and the strand filter (out_off / out_ids), the fragment length KmerIndex::mapPair gives (-1: none),
// the number of distinct non-empty sets its hits carried and the number of distinct shades among them; sets_out (nullable): row i = {1 when the
// item is mapped else 0, the set ids -- with --union the mate flags EC_MATE1 / EC_MATE2 in bits 30 / 31 -- up to sets_stride - 1 of them}.  opts: bit 0 --no-jump, bit 1 --union.
// Returns the number of ids written, -1 when a list overflowed, -2 when out_ids is too small, -3 when the index has no shades.
extern "C" int64_t emu_shade_quant(const kamd_index_view* v, const uint32_t* words, const uint16_t* lens, uint64_t n_items, int paired,
                                   int32_t max_len, int strand, int opts, uint64_t* out_off, uint32_t* out_ids, uint64_t cap, int32_t* tl_out,
                                   uint32_t* n_sets, uint32_t* n_shade_union, uint32_t* sets_out, uint64_t sets_stride) {
  using namespace kamd;
  if (!v->n_shades) return -3;
  const bool no_jump = (opts & 1) != 0, do_union = (opts & 2) != 0;
  const uint64_t sw = (uint64_t)(max_len + 15) / 16 + 1, rec = kamd_packed_record_words(max_len);
  Table t{v->table, v->n_buckets};
  t.layout = (uint8_t)v->table_layout; t.q = (uint8_t)v->tag_q; t.dsh = (uint8_t)v->tag_dsh; t.tagw = (uint8_t)v->tag_w;
  t.dslots = v->dtable; t.n_dbuckets = v->n_dbuckets; t.dummy_uec = v->dummy_uec; t.dummy_slot = v->dummy_slot; t.dummy_strand = v->dummy_strand != 0;
  t.partial = false;   // an index with shades: match(..., partial = false)
  t.no_jump = no_jump;
  const PosTables pt{v->unitig_blk_off, v->unitig_len, v->blk_unitig, v->blk_lb, v->blk_ub, v->blk_ec, v->blk_pos_off, v->blk_posw,
                     v->blk_sense, v->ec_off, v->ec_ids, v->target_lens, v->k};
  const ShadeTables sh{v->core_off, v->core_ids, v->shade_off, v->shade_ids, v->shade_colour};
  std::vector<uint8_t> nonempty(v->n_ecs);
  for (uint64_t e = 0; e < v->n_ecs; e++) nonempty[e] = v->ec_off[e + 1] > v->ec_off[e];
  std::vector<uint32_t> ecbuf(1024), curbuf(1024), hbuf(1024), seen;
  uint64_t o = 0;
  for (uint64_t i = 0; i < n_items; i++) {
    out_off[i] = o; tl_out[i] = -1; n_sets[i] = 0; n_shade_union[i] = 0;
    EcList ecs{ecbuf.data(), 1024, 0, false};
    MateInfo m[2]; memset(m, 0, sizeof m); m[0].first_pos = m[1].first_pos = -1;
    HitBlocks hb{v->slot_block, hbuf.data(), 1024, 0, false};
    for (int mate = 0; mate < (paired ? 2 : 1); mate++) {
      const uint64_t r = paired ? 2 * i + mate : i;
      ReadView rv{words + r * rec, words + r * rec + sw, lens[r]};
      match_mate(t, v->uec_ec, nonempty.data(), rv, v->k, ecs, m[mate], do_union ? (mate ? EC_MATE2 : EC_MATE1) : 0u, (strand && mate == 0) ? &hb : nullptr);
    }
    if (ecs.overflow || hb.overflow) return -1;
    n_sets[i] = (uint32_t)ecs.n;
    seen.clear();
    for (int j = 0; j < ecs.n; j++) { const uint32_t e = ecs.e[j] & EC_ID_MASK; seen.insert(seen.end(), v->shade_ids + v->shade_off[e], v->shade_ids + v->shade_off[e + 1]); }
    std::sort(seen.begin(), seen.end());
    n_shade_union[i] = (uint32_t)(std::unique(seen.begin(), seen.end()) - seen.begin());
    const bool mapped = pair_is_mapped(m[0], m[1]);
    if (sets_out) {
      uint32_t* so = sets_out + i * sets_stride;
      so[0] = mapped ? 1u : 0u;
      for (int j = 0; j < ecs.n && (uint64_t)j + 1 < sets_stride; j++) so[1 + j] = ecs.e[j];
    }
    if (!mapped) continue;
    FirstHit h[2];
    for (int mate = 0; mate < 2; mate++) {
      h[mate].valid = m[mate].n_hits > 0;
      h[mate].block = h[mate].valid ? v->slot_block[m[mate].first_slot] : 0;
      h[mate].dist = h[mate].valid ? v->slot_dist[m[mate].first_slot] : 0;
      h[mate].strand = m[mate].first_strand; h[mate].pos = m[mate].first_pos;
    }
    FilterCfg cfg;
    cfg.fraglen = false; cfg.fl = 0; cfg.strand = strand;
    cfg.comprehensive = strand != 0;   // an index with shades: the strand filter runs per hit
    cfg.hits1 = hbuf.data(); cfg.n_hits1 = hb.n;
    int64_t err = 0;
    for_each_in_shaded_set(sh, ecs, do_union, curbuf.data(), [&](uint32_t tr) {
      if (!(v->onlist_bits[tr >> 5] >> (tr & 31) & 1)) return;
      if (cfg.strand && !keep_transcript(pt, cfg, h[0], h[1], tr)) return;
      if (o >= cap) { err = -2; return; }
      out_ids[o++] = tr;
    });
    if (err) return err;
    if (paired && m[0].n_hits > 0 && m[1].n_hits > 0) {   // KmerIndex::mapPair on the first present k-mers (as k_fld)
      const uint32_t b0 = v->slot_block[m[0].first_slot], b1 = v->slot_block[m[1].first_slot];
      if (b0 == b1 && m[0].first_strand != m[1].first_strand) {
        const int d0 = (int)v->slot_dist[m[0].first_slot], d1 = (int)v->slot_dist[m[1].first_slot];
        const int p1 = m[0].first_strand ? d0 - m[0].first_pos : d0 + v->k + m[0].first_pos;
        const int p2 = m[1].first_strand ? d1 - m[1].first_pos : d1 + v->k + m[1].first_pos;
        tl_out[i] = p1 > p2 ? p1 - p2 : p2 - p1;
      }
    }
  }
  out_off[n_items] = o;
  return (int64_t)o;
}
