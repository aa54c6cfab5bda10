// kamd_ixbuild.h -- what the two builders of the k-mer table share: the host builder of kamd_index.cpp (kamd_index_load) and the device
// builder of kamd_ixbuild.hip (kamd_index_upload on an index loaded with kamd_index_load_deferred).
//
//   * the geometry decisions (host only): the initial number of home buckets from layout and load, the shifts of the compact layout, the
//     fall-back to the wide layout, the growth step while a key lies farther from its home than the displacement field can say;
//   * the per-item steps of the device build as host/device functions (the __global__ kernels are thin wrappers; the CPU build under
//     tests/emu_ixbuild drives the same functions serially): enumeration of the k-mers from the unitig text, the max-plus scan that lays the
//     home groups down in Robin-Hood order, and the reconstruction of a slot from the text position staged for it.
//
// The device build is defined as the table the host builder produces with ONE thread: the keys of a home bucket lie in ascending text
// position.  Everything in the table is then a pure function of slot -> text position.
#pragma once
#include "../../include/kallisto_amd.h"
#include "kamd_core.h"

#include <stdlib.h>

namespace kamd {
namespace ixb {

// ---- geometry -----------------------------------------------------------------------------------------------------------------------
KAMD_HD uint32_t bits_of(uint64_t n) { uint32_t b = 0; while (b < 64 && (n >> b)) ++b; return b; }   // bits that hold the values 0..n
// the shifts of the compact layout for a table of nb home buckets; false: a field does not fit (kamd_core.h)
KAMD_HD bool compact_shifts(int k, uint64_t nb, uint64_t n_uec, uint64_t text_bases, uint32_t* q, uint32_t* dsh, uint32_t* w) {
  *q = compact_q_of(nb);
  *dsh = *q + (uint32_t)(2 * k - 32 > 0 ? 2 * k - 32 : 0);
  *w = *dsh + (*dsh + 4 + bits_of(n_uec) <= 64 ? 4 : 3);   // the displacement: four bits when the class ids leave room for them
  return *w + bits_of(n_uec) <= 64 && text_bases <= COMPACT_GPOS_MASK;
}

struct Geometry {
  int k = 0, want = KAMD_TABLE_AUTO;     // want: KAMD_TABLE_WIDE / _COMPACT / _AUTO as asked for
  uint64_t n_kmers = 0, nb_wide = 0;
  double compact_load = 0.0;             // resolved load factor of the compact table
  // the state the builders iterate on
  bool compact = false;
  uint64_t S = BUCKET_SLOTS, nb = 0;
  uint32_t tag_q = 0, tag_dsh = 0, tag_w = 0;
};
enum { GEO_OK = 0, GEO_RECOUNT = 1, GEO_FAIL = -1 };

// (host functions)
// The footprint up to which dependent random reads run at full rate is a property of the device (MI355X: 2.4 GB), not of the library:
// KAMD_TABLE_KNEE_GB overrides it for another part.
inline double table_knee_bytes() {
  double knee = 2.4e9;
  if (const char* e = getenv("KAMD_TABLE_KNEE_GB")) { const double v = atof(e); if (v > 0.05 && v < 1024.0) knee = v * 1e9; }
  return knee;
}
// load factor when the caller names none: the sparsest of 0.4 / 0.5 whose table stays under the knee, 0.6 beyond
inline double default_compact_load(uint64_t n_kmers, double knee) {
  const double bytes_at_1 = (double)n_kmers * (64.0 / COMPACT_SLOTS);
  return bytes_at_1 / 0.4 <= knee ? 0.4 : bytes_at_1 / 0.5 <= knee ? 0.5 : 0.6;
}
// the table both builders start from: wide = 3 slots per line at a load of 0.5; compact = 4 slots at `load_arg` when it lies in [0.2, 0.9],
// else at the default load.  false: too many k-mers for 32-bit bucket numbers
inline bool geometry_init(Geometry& g, int k, uint64_t n_kmers, int want, double load_arg) {
  g.k = k; g.want = want; g.n_kmers = n_kmers;
  g.compact_load = (load_arg >= 0.2 && load_arg <= 0.9) ? load_arg : default_compact_load(n_kmers, table_knee_bytes());
  g.compact = want != KAMD_TABLE_WIDE;
  const uint64_t wide = (n_kmers * 2 + BUCKET_SLOTS - 1) / BUCKET_SLOTS;   // load factor 0.5 over 3-slot buckets
  g.nb_wide = wide > 16 ? wide : 16;
  g.S = g.compact ? COMPACT_SLOTS : BUCKET_SLOTS;
  if (g.compact) { const uint64_t c = (uint64_t)((double)n_kmers / g.compact_load / (double)g.S) + 1; g.nb = c > 16 ? c : 16; }
  else g.nb = g.nb_wide;
  g.tag_q = g.tag_dsh = g.tag_w = 0;
  return (g.nb > g.nb_wide ? g.nb : g.nb_wide) < 0xF0000000ULL;
}
// in front of a scan: the compact layout must hold the class ids and the text positions beside the tag.  GEO_FAIL: it cannot and was asked
// for by name; GEO_RECOUNT: it cannot, the wide table is built instead (its home buckets have to be counted); GEO_OK: go on
inline int geometry_fit(Geometry& g, uint64_t n_uec, uint64_t text_bases) {
  if (!g.compact || compact_shifts(g.k, g.nb, n_uec, text_bases, &g.tag_q, &g.tag_dsh, &g.tag_w)) return GEO_OK;
  if (g.want == KAMD_TABLE_COMPACT) return GEO_FAIL;
  g.compact = false; g.S = BUCKET_SLOTS; g.nb = g.nb_wide;
  return GEO_RECOUNT;
}
// behind a scan: a key must lie no farther from its home than the displacement field can say (14 or 6 buckets), otherwise a sixteenth
// more buckets and the count again
inline int geometry_after_scan(Geometry& g, uint64_t max_disp) {
  if (!g.compact || max_disp <= (uint64_t)((1u << (g.tag_w - g.tag_dsh)) - 2u)) return GEO_OK;
  g.nb += g.nb / 16 + 1;
  return GEO_RECOUNT;
}
inline uint64_t total_buckets_of(uint64_t nb, uint64_t end_cursor, uint64_t S) { const uint64_t used = (end_cursor + S - 1) / S; return (nb > used ? nb : used) + 1; }
inline uint64_t dlist_home_buckets(uint64_t n_keys) { const uint64_t b = (n_keys * 2 + BUCKET_SLOTS - 1) / BUCKET_SLOTS; return b > 16 ? b : 16; }

// ---- the scan ------------------------------------------------------------------------------------------------------------------------
// base[b] = max(end[b-1], b*S), end[b] = base[b] + fill[b].  With x[b] = end[b] - (b+1)*S it reads x[b] = max(x[b-1], 0) + fill[b] - S, a
// map x -> max(x + a, m) with a = m = fill[b] - S; such maps compose associatively, so the recurrence is a scan.  x[-1] = 0.
struct ScanOp { int64_t a, m; };
static const int64_t SCAN_NEG = -(1LL << 60);
KAMD_HD ScanOp scan_identity() { return ScanOp{0, SCAN_NEG}; }
KAMD_HD ScanOp scan_op_of(uint32_t fill, uint32_t S) { const int64_t c = (int64_t)fill - (int64_t)S; return ScanOp{c, c}; }
KAMD_HD ScanOp scan_compose(const ScanOp& first, const ScanOp& then) {   // x -> then(first(x))
  const int64_t m = first.m + then.a;
  return ScanOp{first.a + then.a, m > then.m ? m : then.m};
}
KAMD_HD int64_t scan_apply(const ScanOp& f, int64_t x) { const int64_t y = x + f.a; return y > f.m ? y : f.m; }
// one bucket, given the x that enters it: where its home group starts, where it ends; x becomes the x that leaves it
struct ScanOut { uint64_t base, end; };
KAMD_HD ScanOut scan_bucket(int64_t& x, uint64_t b, uint32_t fill, uint32_t S) {
  const int64_t x0 = x > 0 ? x : 0;
  ScanOut o;
  o.base = b * S + (uint64_t)x0;
  x = x0 + (int64_t)fill - (int64_t)S;
  o.end = o.base + fill;
  return o;
}
KAMD_HD uint64_t bucket_disp(uint64_t end, uint64_t b, uint32_t S) { return (end - 1) / S - b; }   // of a bucket with fill > 0

// ---- enumeration of the k-mers from the unitig text ------------------------------------------------------------------------------------
struct TextView {
  const uint32_t* utext;         // + two words of padding
  const uint64_t* unitig_gpos;   // [n_unitigs + 1], strictly increasing (a unitig holds at least k bases)
  uint64_t n_unitigs, text_bases;
  int k;
};
// the unitig that holds text position g < text_bases: the last u with unitig_gpos[u] <= g
KAMD_HD uint64_t unitig_of(const TextView& t, uint64_t g) {
  uint64_t lo = 0, hi = t.n_unitigs;   // answer in [lo, hi)
  while (hi - lo > 1) { const uint64_t mid = lo + ((hi - lo) >> 1); if (t.unitig_gpos[mid] <= g) lo = mid; else hi = mid; }
  return lo;
}
// the same, walking forward from a unitig known to start at or before g
KAMD_HD uint64_t unitig_from(const TextView& t, uint64_t u, uint64_t g) {
  while (u + 1 < t.n_unitigs && t.unitig_gpos[u + 1] <= g) ++u;
  return u;
}
struct TextKmer { uint64_t canon; bool fwd_is_canon; };
KAMD_HD TextKmer text_kmer(const uint32_t* utext, uint32_t g, int k) {
  const TextWords w = load_text(utext, g);
  const int sh = (int)(g & 15u) * 2;
  uint64_t x = ((uint64_t)w.a | ((uint64_t)w.b << 32)) >> sh;
  if (sh + 2 * k > 64) x |= (uint64_t)w.c << (64 - sh);
  x &= (k == 32) ? ~0ULL : ((1ULL << (2 * k)) - 1);
  const uint64_t fwd = rev_bases64(x) >> (64 - 2 * k);
  const uint64_t rc = revcomp_msb(fwd, k);
  return TextKmer{fwd < rc ? fwd : rc, fwd < rc};
}
// text position g of unitig u: does a k-mer start there, and in which home bucket of a table of nb does it live?
KAMD_HD bool kmer_home(const TextView& t, uint64_t u, uint64_t g, uint64_t nb, uint64_t* hb) {
  if (g + (uint64_t)t.k > t.unitig_gpos[u + 1]) return false;
  *hb = home_bucket(text_kmer(t.utext, (uint32_t)g, t.k).canon, nb);
  return true;
}

// ---- a slot from the text position staged for it ---------------------------------------------------------------------------------------
static const uint32_t STAGE_EMPTY = 0xFFFFFFFFu;
struct FillView {
  TextView text;
  const uint64_t* unitig_blk_off; const uint32_t* blk_lb; const uint32_t* blk_ub; const uint32_t* blk_uec;
  uint64_t n_blocks;
  const uint64_t* base;            // [nb]: first slot of every home group
  uint64_t nb, total_buckets, end_cursor;
  uint32_t S, layout, tag_q, tag_dsh, tag_w;
  const uint64_t* keys;            // D-list table: the staged values index this list of canonical keys (sorted, distinct) instead of the text
  uint64_t n_keys;
};
// a bucket continues into the next one when keys homed at or before it spill past its slots
KAMD_HD bool bucket_continues(const FillView& f, uint64_t b) {
  const uint64_t reach = b + 1 < f.nb ? f.base[b + 1] : f.end_cursor;
  return reach > (b + 1) * f.S;
}
// slot s of `table` (total_buckets x 8 words), slot_block[s], slot_dist[s] (both null for the D-list table) from staged = the text position
// of the slot's k-mer, or STAGE_EMPTY.  The last bucket is the pad that ends every probe: it stays empty whatever was staged.
KAMD_HD void fill_slot(const FillView& f, uint64_t s, uint32_t staged, uint64_t* table, uint32_t* slot_block, uint32_t* slot_dist) {
  const uint64_t bk = s / f.S, j = s % f.S;
  uint64_t* w = table + 8 * bk;
  bool occupied = staged != STAGE_EMPTY && bk + 1 < f.total_buckets;
  if (occupied) occupied = f.keys ? staged < f.n_keys : (uint64_t)staged + (uint64_t)f.text.k <= f.text.text_bases;
  uint64_t cn = 0, payload = 0; uint32_t gpos = 0, block = 0xFFFFFFFFu, dist = 0;
  if (occupied && f.keys) cn = f.keys[staged];
  else if (occupied) {
    const uint64_t u = unitig_of(f.text, staged);
    const uint64_t b0 = f.unitig_blk_off[u], b1 = f.unitig_blk_off[u + 1];
    if (b0 < b1 && b1 <= f.n_blocks) {
      dist = (uint32_t)(staged - f.text.unitig_gpos[u]);
      // block containing dist: BlockArray::get_block_at = last block with lb <= dist (the blocks of a unitig are sorted by lb)
      uint64_t lo = b0, hi = b1;
      while (hi - lo > 1) { const uint64_t mid = lo + ((hi - lo) >> 1); if (f.blk_lb[mid] <= dist) lo = mid; else hi = mid; }
      const TextKmer tk = text_kmer(f.text.utext, staged, f.text.k);
      const uint32_t lb = f.blk_lb[lo], ub = f.blk_ub[lo];
      cn = tk.canon; gpos = staged; block = (uint32_t)lo;
      payload = make_payload(ub - 1 - dist, dist - lb, f.blk_uec[lo], tk.fwd_is_canon);   // KmerIndex.cpp:1780-1789
    } else occupied = false;
  }
  const bool cont = occupied && j == 0 && bucket_continues(f, bk);
  if (f.layout == (uint32_t)LAYOUT_COMPACT) {
    if (!occupied) { w[2 * j] = ~0ULL; w[2 * j + 1] = 0; }   // displacement all ones = empty
    else {
      Table t{nullptr, f.nb};
      t.layout = (uint8_t)LAYOUT_COMPACT; t.q = (uint8_t)f.tag_q; t.dsh = (uint8_t)f.tag_dsh; t.tagw = (uint8_t)f.tag_w;
      const uint32_t h = kmer_hash32(cn);
      const uint64_t uec = (payload >> 32) & 0x7FFFFFFFULL;
      w[2 * j] = compact_tag(t, cn, h, (uint32_t)(bk - bucket_of_hash(h, f.nb))) | (uec << f.tag_w);
      w[2 * j + 1] = (payload & 0xFFFFFFFFULL) | ((uint64_t)gpos << 32) | ((payload >> 63) ? COMPACT_FWD : 0ULL) | (cont ? COMPACT_CONT : 0ULL);
    }
  } else {
    w[j] = !occupied ? KEY_EMPTY : cont ? (cn | KEY_CONT) : cn;
    w[f.S + j] = payload;
    uint32_t* gp = reinterpret_cast<uint32_t*>(w + 2 * f.S);
    gp[j] = gpos;
    if (j + 1 == f.S) gp[f.S] = 0;   // the line's four spare bytes
  }
  if (slot_block) slot_block[s] = occupied ? block : 0xFFFFFFFFu;
  if (slot_dist) slot_dist[s] = dist;
}
// the staged positions of one home group in ascending order (what one thread enumerating the unitigs in order lays down)
KAMD_HD void order_group(uint32_t* staged, uint32_t n) {
  for (uint32_t i = 1; i < n; i++) {
    const uint32_t x = staged[i];
    uint32_t j = i;
    while (j > 0 && staged[j - 1] > x) { staged[j] = staged[j - 1]; --j; }
    staged[j] = x;
  }
}

}  // namespace ixb
}  // namespace kamd

// ---- what the device builder needs of a kamd_index beyond its view (kamd_index.cpp; internal, not part of the C ABI) ---------------------------
struct kamd_index;
struct kamd_ixbuild_info {
  int deferred;                 // loaded by kamd_index_load_deferred: the tables are to be built by kamd_index_upload
  int layout; double load;      // the layout and load factor asked for
  const uint32_t* blk_uec;      // per block: its (unitig, transcript-set) class
  const uint64_t* dlist_keys;   // [dlist_size] canonical keys; [0] = the dummy
};
extern "C" int kamd_ixbuild_info_get(const kamd_index*, kamd_ixbuild_info* out);
