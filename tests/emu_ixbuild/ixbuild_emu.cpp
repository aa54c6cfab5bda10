// TEST INFRASTRUCTURE: the steps of the device index builder (kallisto_amd/csrc/kamd_ixbuild.hip) run serially on the CPU through the very
// host/device functions the kernels wrap (kamd_ixbuild.h).  What a GPU does in an order nobody controls is made awkward on purpose: the scan
// combines its maps over chunks of a size the caller picks (7, say), the placement runs over the items in REVERSED order, so that the
// ordering step has work to do.
#include "../../include/kallisto_amd.h"
#include "../../kallisto_amd/csrc/kamd_core.h"
#include "../../kallisto_amd/csrc/kamd_ixbuild.h"

#include <algorithm>
#include <cstring>
#include <vector>

namespace ixb = kamd::ixb;

namespace {
// base[nb], end_cursor, max_disp from fill[nb]: per-chunk reduce, scan of the chunk summaries, apply
void scan_chunked(const uint32_t* fill, uint64_t nb, uint32_t S, uint64_t chunk, uint64_t* base, uint64_t* end_cursor, uint64_t* max_disp) {
  const uint64_t nc = (nb + chunk - 1) / chunk;
  std::vector<ixb::ScanOp> sums(nc);
  for (uint64_t c = 0; c < nc; c++) {
    ixb::ScanOp op = ixb::scan_identity();
    for (uint64_t b = c * chunk; b < std::min(nb, (c + 1) * chunk); b++) op = ixb::scan_compose(op, ixb::scan_op_of(fill[b], S));
    sums[c] = op;
  }
  // (the summaries are themselves combined pairwise from the right end first and then applied: associativity, not a running value)
  std::vector<ixb::ScanOp> prefix(nc + 1);
  prefix[0] = ixb::scan_identity();
  for (uint64_t c = 0; c < nc; c++) prefix[c + 1] = c % 2 ? ixb::scan_compose(prefix[c - 1], ixb::scan_compose(sums[c - 1], sums[c])) : ixb::scan_compose(prefix[c], sums[c]);
  uint64_t md = 0, end = 0;
  for (uint64_t c = 0; c < nc; c++) {
    int64_t x = ixb::scan_apply(prefix[c], 0);
    for (uint64_t b = c * chunk; b < std::min(nb, (c + 1) * chunk); b++) {
      const ixb::ScanOut o = ixb::scan_bucket(x, b, fill[b], S);
      base[b] = o.base;
      if (fill[b]) md = std::max(md, ixb::bucket_disp(o.end, b, S));
      if (b + 1 == nb) end = o.end;
    }
  }
  *end_cursor = end; *max_disp = md;
}
// items: text positions (keys == null) or D-list keys
bool item_home(const ixb::TextView& tv, const uint64_t* keys, uint64_t i, uint64_t nb, uint64_t* hb) {
  if (keys) { *hb = kamd::home_bucket(keys[i], nb); return true; }
  const uint64_t u = ixb::unitig_from(tv, ixb::unitig_of(tv, i & ~(uint64_t)63), i);   // as a wavefront does
  return ixb::kmer_home(tv, u, i, nb, hb);
}
void count(const ixb::TextView& tv, const uint64_t* keys, uint64_t n_items, uint64_t nb, std::vector<uint32_t>& fill) {
  fill.assign(nb + 1, 0);
  for (uint64_t i = 0; i < n_items; i++) { uint64_t hb; if (item_home(tv, keys, i, nb, &hb)) ++fill[hb]; }
}
void place_order_fill(ixb::FillView f, uint64_t n_items, const std::vector<uint32_t>& fill, bool reversed, uint64_t* table, uint32_t* slot_block, uint32_t* slot_dist) {
  const uint64_t total = f.total_buckets * f.S;
  std::vector<uint32_t> staged(total, ixb::STAGE_EMPTY), fill2(f.nb + 1, 0);
  for (uint64_t n = 0; n < n_items; n++) {
    const uint64_t i = reversed ? n_items - 1 - n : n;
    uint64_t hb;
    if (!item_home(f.text, f.keys, i, f.nb, &hb)) continue;
    const uint64_t slot = f.base[hb] + fill2[hb]++;
    if (slot < total) staged[slot] = (uint32_t)i;
  }
  for (uint64_t b = 0; b < f.nb; b++) if (fill[b] >= 2 && f.base[b] + fill[b] <= total) ixb::order_group(staged.data() + f.base[b], fill[b]);
  for (uint64_t s = 0; s < total; s++) ixb::fill_slot(f, s, staged[s], table, slot_block, slot_dist);
}
}  // namespace

extern "C" {
struct ixb_emu_out {
  uint64_t n_buckets, pad_buckets, n_dbuckets, dpad_buckets, dummy_slot;
  uint32_t layout, slots, tag_q, tag_dsh, tag_w, dummy_uec, dummy_strand;
  int32_t rounds;
  uint64_t* table; uint32_t* slot_block; uint32_t* slot_dist; uint64_t* dtable;
};
void ixb_emu_free(ixb_emu_out* o) {
  delete[] o->table; delete[] o->slot_block; delete[] o->slot_dist; delete[] o->dtable;
  o->table = o->dtable = nullptr; o->slot_block = o->slot_dist = nullptr;
}
// 0 ok, -3 as the builders fail
int ixb_emu_build(const kamd_index* ix, uint64_t chunk, int reversed, ixb_emu_out* o) {
  memset(o, 0, sizeof *o);
  kamd_index_view v; kamd_ixbuild_info bi;
  if (kamd_index_get_view(ix, &v) || kamd_ixbuild_info_get(ix, &bi) || chunk == 0) return -1;
  const ixb::TextView tv{v.utext, v.unitig_gpos, v.n_unitigs, v.text_bases, v.k};
  ixb::Geometry geo;
  if (!ixb::geometry_init(geo, v.k, v.n_kmers, bi.layout, bi.load)) return -3;
  std::vector<uint32_t> fill; std::vector<uint64_t> base;
  uint64_t end_cursor = 0, max_disp = 0;
  for (;;) {
    if (ixb::geometry_fit(geo, v.n_uec, v.text_bases) == ixb::GEO_FAIL) return -3;
    count(tv, nullptr, v.text_bases, geo.nb, fill);
    base.assign(geo.nb, 0);
    scan_chunked(fill.data(), geo.nb, (uint32_t)geo.S, chunk, base.data(), &end_cursor, &max_disp);
    ++o->rounds;
    if (ixb::geometry_after_scan(geo, max_disp) == ixb::GEO_OK) break;
  }
  const uint64_t tb = ixb::total_buckets_of(geo.nb, end_cursor, geo.S);
  o->n_buckets = geo.nb; o->pad_buckets = tb - geo.nb; o->layout = geo.compact ? kamd::LAYOUT_COMPACT : kamd::LAYOUT_WIDE; o->slots = (uint32_t)geo.S;
  o->tag_q = geo.compact ? geo.tag_q : 0; o->tag_dsh = geo.compact ? geo.tag_dsh : 0; o->tag_w = geo.compact ? geo.tag_w : 0;
  o->table = new uint64_t[tb * 8]; o->slot_block = new uint32_t[tb * geo.S]; o->slot_dist = new uint32_t[tb * geo.S];
  memset(o->table, 0xAB, tb * 64); memset(o->slot_block, 0xAB, tb * geo.S * 4); memset(o->slot_dist, 0xAB, tb * geo.S * 4);   // (every byte must be written)
  ixb::FillView f{};
  f.text = tv; f.unitig_blk_off = v.unitig_blk_off; f.blk_lb = v.blk_lb; f.blk_ub = v.blk_ub; f.blk_uec = bi.blk_uec; f.n_blocks = v.n_blocks;
  f.base = base.data(); f.nb = geo.nb; f.total_buckets = tb; f.end_cursor = end_cursor; f.S = (uint32_t)geo.S; f.layout = o->layout;
  f.tag_q = o->tag_q; f.tag_dsh = o->tag_dsh; f.tag_w = o->tag_w;
  place_order_fill(f, v.text_bases, fill, reversed != 0, o->table, o->slot_block, o->slot_dist);
  if (v.dlist_size) {
    std::vector<uint64_t> keys(bi.dlist_keys, bi.dlist_keys + v.dlist_size);
    std::sort(keys.begin(), keys.end());
    keys.erase(std::unique(keys.begin(), keys.end()), keys.end());
    const uint64_t ndb = ixb::dlist_home_buckets(v.dlist_size);
    std::vector<uint32_t> dfill; std::vector<uint64_t> dbase(ndb);
    uint64_t dend = 0, ddisp = 0;
    count(tv, keys.data(), keys.size(), ndb, dfill);
    scan_chunked(dfill.data(), ndb, kamd::BUCKET_SLOTS, chunk, dbase.data(), &dend, &ddisp);
    const uint64_t dtb = ixb::total_buckets_of(ndb, dend, kamd::BUCKET_SLOTS);
    o->n_dbuckets = ndb; o->dpad_buckets = dtb - ndb;
    o->dtable = new uint64_t[dtb * 8];
    memset(o->dtable, 0xAB, dtb * 64);
    ixb::FillView g{};
    g.text = tv; g.base = dbase.data(); g.nb = ndb; g.total_buckets = dtb; g.end_cursor = dend; g.S = kamd::BUCKET_SLOTS; g.layout = kamd::LAYOUT_WIDE;
    g.keys = keys.data(); g.n_keys = keys.size();
    place_order_fill(g, keys.size(), dfill, reversed != 0, o->dtable, nullptr, nullptr);
    kamd::Table t{o->table, geo.nb};
    t.layout = (uint8_t)o->layout; t.q = (uint8_t)o->tag_q; t.dsh = (uint8_t)o->tag_dsh; t.tagw = (uint8_t)o->tag_w;
    const kamd::Probe p = kamd::probe_table(t, bi.dlist_keys[0], true, nullptr);
    if (!p.found) { ixb_emu_free(o); return -3; }
    o->dummy_slot = p.slot; o->dummy_uec = p.uec; o->dummy_strand = p.strand ? 1 : 0;
  }
  return 0;
}
int ixb_emu_scan(const uint32_t* fill, uint64_t nb, uint32_t S, uint64_t chunk, uint64_t* base, uint64_t* end_cursor, uint64_t* max_disp) {
  if (!chunk) return -1;
  scan_chunked(fill, nb, S, chunk, base, end_cursor, max_disp);
  return 0;
}
// the geometry decisions, one call per decision: g = {compact, S, nb, tag_q, tag_dsh, tag_w, nb_wide}
static void geo_out(const ixb::Geometry& g, uint64_t* o) { o[0] = g.compact; o[1] = g.S; o[2] = g.nb; o[3] = g.tag_q; o[4] = g.tag_dsh; o[5] = g.tag_w; o[6] = g.nb_wide; }
void* ixb_emu_geo_new(int k, uint64_t n_kmers, int want, double load, int* ok, uint64_t* o) {
  ixb::Geometry* g = new ixb::Geometry;
  *ok = ixb::geometry_init(*g, k, n_kmers, want, load) ? 1 : 0;
  geo_out(*g, o);
  return g;
}
int ixb_emu_geo_fit(void* h, uint64_t n_uec, uint64_t text_bases, uint64_t* o) { ixb::Geometry* g = (ixb::Geometry*)h; const int r = ixb::geometry_fit(*g, n_uec, text_bases); geo_out(*g, o); return r; }
int ixb_emu_geo_after_scan(void* h, uint64_t max_disp, uint64_t* o) { ixb::Geometry* g = (ixb::Geometry*)h; const int r = ixb::geometry_after_scan(*g, max_disp); geo_out(*g, o); return r; }
void ixb_emu_geo_free(void* h) { delete (ixb::Geometry*)h; }
uint64_t ixb_emu_total_buckets(uint64_t nb, uint64_t end_cursor, uint64_t S) { return ixb::total_buckets_of(nb, end_cursor, S); }
}
