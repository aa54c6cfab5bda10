// kamd_aa.h -- per-item logic of the translated search (`bus --aa`), host/device inline like kamd_core.h: the kernels of
// kamd_aa.hip and the CPU emulation of tests/emu_aa drive exactly these functions.
//
// Reference semantics restated here (file:line in the reference tree):
//   six frames, match per frame      src/ProcessReads.cpp:1633-1726
//   nn_to_cfc / cfc_map              src/KmerIndex.cpp:16-138 (standard genetic code, then cfc_aa_map of src/common.cpp)
//   KmerIndex::match with cfc        src/KmerIndex.cpp:1698-1940 (`l` stays the untranslated length, :1734-1737)
//   intersectECs with dfk_onlist     src/MinCollector.cpp:425-496, includeDList :37-42
//   intersectKmersCFC                src/MinCollector.cpp:44-119
#pragma once
#include "kamd_core.h"

namespace kamd {

// ---------------------------------------------------------------------------------------------------------------
// codon -> comma-free triplet.  Codon index = b0 * 16 + b1 * 4 + b2 with A = 0, C = 1, G = 2, T = 3 (the reads' 2-bit codes);
// value = t0 | t1 << 2 | t2 << 4, or CFC_MASKED for the three stop codons ("NNN": three masked bases).
// ---------------------------------------------------------------------------------------------------------------
static const uint32_t CFC_MASKED = 0xFFu;
KAMD_HD uint32_t cfc_of_codon(uint32_t codon) {
  constexpr uint8_t T[64] = {
      //  AAA K  AAC N  AAG K  AAT N  ACA T  ACC T  ACG T  ACT T  AGA R  AGC S  AGG R  AGT S  ATA I  ATC I  ATG M  ATT I
      0x19, 0x09, 0x19, 0x09, 0x3D, 0x3D, 0x3D, 0x3D, 0x3B, 0x0D, 0x3B, 0x0D, 0x0C, 0x0C, 0x1C, 0x0C,
      //  CAA Q  CAC H  CAG Q  CAT H  CCA P  CCC P  CCG P  CCT P  CGA R  CGC R  CGG R  CGT R  CTA L  CTC L  CTG L  CTT L
      0x28, 0x38, 0x28, 0x38, 0x1D, 0x1D, 0x1D, 0x1D, 0x3B, 0x3B, 0x3B, 0x3B, 0x04, 0x04, 0x04, 0x04,
      //  GAA E  GAC D  GAG E  GAT D  GCA A  GCC A  GCG A  GCT A  GGA G  GGC G  GGG G  GGT G  GTA V  GTC V  GTG V  GTT V
      0x29, 0x39, 0x29, 0x39, 0x08, 0x08, 0x08, 0x08, 0x2B, 0x2B, 0x2B, 0x2B, 0x3C, 0x3C, 0x3C, 0x3C,
      //  TAA *  TAC Y  TAG *  TAT Y  TCA S  TCC S  TCG S  TCT S  TGA *  TGC C  TGG W  TGT C  TTA L  TTC F  TTG L  TTT F
      0xFF, 0x18, 0xFF, 0x18, 0x0D, 0x0D, 0x0D, 0x0D, 0xFF, 0x0B, 0x1B, 0x0B, 0x04, 0x14, 0x04, 0x14};
  return T[codon & 63u];
}

// ---------------------------------------------------------------------------------------------------------------
// frames.  Frame f of a read s of l bases: f < 3: s + f; f >= 3: rc(s) + (f - 3).  l_f = l - f % 3 bases, of which the
// 3 * floor(l_f / 3) that fill codons are translated.  A codon with a non-ACGT base translates to three masked bases.
// ---------------------------------------------------------------------------------------------------------------
static const int AA_FRAMES = 6;
KAMD_HD int aa_frame_len(int l, int f) { const int lf = l - f % 3; return lf > 0 ? lf : 0; }
KAMD_HD int aa_translated_len(int l, int f) { return aa_frame_len(l, f) / 3 * 3; }

// base p of frame f as 2-bit code, 4 = not ACGT (the reverse-complement frames read the source backwards)
KAMD_HD uint32_t aa_frame_base(const uint32_t* seq, const uint32_t* mask, int l, int f, int p) {
  const int i = f < 3 ? p + f : l - 1 - (p + f - 3);
  if ((mask[i >> 5] >> (i & 31)) & 1u) return 4u;
  const uint32_t b = (seq[i >> 4] >> (2 * (i & 15))) & 3u;
  return f < 3 ? b : 3u - b;
}
// triplet of codon c of frame f (CFC_MASKED: stop codon or a non-ACGT base)
KAMD_HD uint32_t aa_frame_codon(const uint32_t* seq, const uint32_t* mask, int l, int f, int c) {
  const uint32_t b0 = aa_frame_base(seq, mask, l, f, 3 * c), b1 = aa_frame_base(seq, mask, l, f, 3 * c + 1), b2 = aa_frame_base(seq, mask, l, f, 3 * c + 2);
  if ((b0 | b1 | b2) & 4u) return CFC_MASKED;
  return cfc_of_codon(b0 * 16u + b1 * 4u + b2);
}
// Word `widx` of the packed record (kamd_core.h ReadView: seq_words 2-bit words, the last of them the flag word, then the mask
// words) of frame f's translation.  One caller owns one output word and gathers the codons it covers: up to seven for a
// sequence word (16 bases), twelve for a mask word (32 bases).  The flag word always says "consult the mask plane": a frame
// without a stop codon is the exception.
KAMD_HD uint32_t aa_frame_word(const uint32_t* seq, const uint32_t* mask, int l, int f, int widx, int seq_words) {
  if (widx == seq_words - 1) return REC_FLAG_HAS_N;
  const int tl = aa_translated_len(l, f);
  const bool is_mask = widx >= seq_words;
  const int per = is_mask ? 32 : 16;
  const int q0 = (is_mask ? widx - seq_words : widx) * per;   // first translated base of the word
  if (q0 >= tl) return 0u;
  const int q1 = q0 + per < tl ? q0 + per : tl;
  uint32_t w = 0;
  for (int c = q0 / 3; 3 * c < q1; c++) {
    const uint32_t t = aa_frame_codon(seq, mask, l, f, c);
    for (int e = 0; e < 3; e++) {
      const int q = 3 * c + e;
      if (q < q0 || q >= q1) continue;
      if (is_mask) w |= (t == CFC_MASKED ? 1u : 0u) << (q - q0);
      else if (t != CFC_MASKED) w |= ((t >> (2 * e)) & 3u) << (2 * (q - q0));
    }
  }
  return w;
}

// ---------------------------------------------------------------------------------------------------------------
// the (unitig, set) classes of one frame's hits, kept in the order intersectECs visits them: ascending unitig id (the sort
// of MinCollector.cpp:430-439), classes of one unitig in the order of their first hit.  entry = unitig << 32 | set id
// ---------------------------------------------------------------------------------------------------------------
struct AaClassList {
  uint64_t* e; int stride; int cap; int n; bool overflow;   // stride: distance between entries (lane-interleaved scratch on the device)
};
KAMD_HD void aa_classlist_add(AaClassList& l, uint32_t unitig, uint32_t ec) {
  const uint64_t x = ((uint64_t)unitig << 32) | ec;
  int i = 0;
  for (; i < l.n; i++) {
    const uint64_t y = l.e[i * l.stride];
    if (y == x) return;
    if ((uint32_t)(y >> 32) > unitig) break;
  }
  if (l.n == l.cap) { l.overflow = true; return; }
  for (int j = l.n; j > i; --j) l.e[j * l.stride] = l.e[(j - 1) * l.stride];
  l.e[i * l.stride] = x;
  ++l.n;
}

// what the frame matcher needs of the index beside the k-mer table
struct AaIndex {
  const uint32_t* uec_ec; const uint8_t* ec_nonempty;
  const uint32_t* slot_block; const uint32_t* blk_unitig;   // slot -> block -> unitig: the unitig id of a hit
};
// KmerIndex::match(s, l_f, v, partial = false, cfc = true) for one translated frame: match_mate's logic (kamd_core.h) with two
// lengths -- the windows are those of the translation `r` (r.len bases), the jump clamp and the fake last position use the
// untranslated frame length lf (KmerIndex.cpp:1734-1737 replace s, not l) -- collecting the classes with a non-empty set.
KAMD_HD void aa_match_frame(const Table& t, const AaIndex& ax, const ReadView& r, int lf, int k, AaClassList& cl, uint32_t* probes) {
  const int l = lf;
  uint32_t last_uec = NO_UEC;
  uint32_t np = 0;
#define KAMD_AA_PUSH(P)                                                            \
  do {                                                                             \
    if ((P).uec != last_uec) {                                                     \
      last_uec = (P).uec;                                                          \
      const uint32_t ec_ = ax.uec_ec[(P).uec];                                     \
      if (ax.ec_nonempty[ec_]) aa_classlist_add(cl, ax.blk_unitig[ax.slot_block[(P).slot]], ec_); \
    }                                                                              \
  } while (0)
  int w = next_valid_window(r, 0, k);
  while (w >= 0) {
    bool fc; const uint64_t canon = window_canon(r, w, k, &fc);
    ++np;
    const Probe um = probe_table(t, canon, fc, nullptr);
    if (um.found) {
      const int pos = w;
      KAMD_AA_PUSH(um);                                                            // KmerIndex.cpp:1774
      const int dist = (int)um.dist;                                               // :1789
      if (dist >= 2) {                                                             // :1792 (--no-jump is refused with --aa)
        int nextPos = pos + dist;
        if (pos + dist >= l - k) nextPos = l - k;                                  // :1796-1799, l = lf
        const int w2 = advance_window(r, w, nextPos - pos, k);                     // :1802-1803: beyond the last window of the translation -> end
        if (w2 < 0) break;                                                         // :1882-1886
        bool fc2; const uint64_t c2 = window_canon(r, w2, k, &fc2);
        ++np;
        const Probe um2 = probe_table(t, c2, fc2, nullptr);
        bool found2 = false; int found2pos = pos + dist;
        if (!um2.found) { found2 = true; found2pos = pos; }                        // :1807-1809
        else if (um2.uec == um.uec) { found2 = true; }                             // :1810-1815
        if (found2) {
          if (found2pos >= l - k) break;                                           // :1819-1822 (um's class is in the list)
          w = w2;                                                                  // :1823-1826
        } else {
          bool foundMiddle = false;
          if (dist > 4) {                                                          // :1831
            const int middlePos = (pos + nextPos) / 2;
            const int w3 = advance_window(r, w, middlePos - pos, k);
            if (w3 >= 0) {
              bool fc3; const uint64_t c3 = window_canon(r, w3, k, &fc3);
              ++np;
              const Probe um3 = probe_table(t, c3, fc3, nullptr);
              if (um3.found && (um3.uec == um.uec || um3.uec == um2.uec)) {        // :1842-1850
                foundMiddle = true;
                KAMD_AA_PUSH(um3);                                                 // :1866
                if (nextPos >= l - k) break;                                       // :1867-1868
                w = w2;                                                            // :1870
              }
            }
          }
          if (!foundMiddle) {                                                      // :1876-1925: one-step back-off
            w = next_valid_window(r, w + 1, k);
            if (w < 0) break;
            bool fc4; const uint64_t c4 = window_canon(r, w, k, &fc4);
            ++np;
            const Probe um4 = probe_table(t, c4, fc4, nullptr);
            if (um4.found) KAMD_AA_PUSH(um4);
          }
        }
      }
    }
    w = next_valid_window(r, w + 1, k);
  }
  // D-list (:1928-1939; partial = false: scanned whether or not the frame has hits)
  if (t.n_dbuckets) {
    const Table dt{t.dslots, t.n_dbuckets};
    for (int wd = next_valid_window(r, 0, k); wd >= 0; wd = next_valid_window(r, wd + 1, k)) {
      bool fcd; const uint64_t cd = window_canon(r, wd, k, &fcd);
      if (probe_table(dt, cd, fcd, nullptr).found) {
        Probe dm; dm.found = true; dm.strand = t.dummy_strand; dm.uec = t.dummy_uec; dm.dist = 0; dm.slot = t.dummy_slot; dm.gpos = 0;
        KAMD_AA_PUSH(dm);
        break;
      }
    }
  }
#undef KAMD_AA_PUSH
  if (probes) *probes += np;
}

// ---------------------------------------------------------------------------------------------------------------
// intersectECs with dfk_onlist for one frame.  Before every `r &= ec`, includeDList adds the id n_targets (itself off-list) to
// both when either holds an off-list target: an off-list member is sticky -- once a visited set carries one, r keeps one and can
// no longer run empty -- while r is returned at once when it runs empty before such a set is reached.  With j = the first class
// whose set has an off-list member (ec_offlist, one bit per set computed when the index is uploaded):
//   no such class                      -> r = the intersection of all sets (all on-list)
//   j == 0, or sets [0, j) intersect   -> r has an off-list member: the READ is rejected (intersectKmersCFC, :53-64)
//   sets [0, j) do not intersect       -> r = {} by the early return, the classes from j on are never visited
// ---------------------------------------------------------------------------------------------------------------
struct AaFrameSet {
  uint32_t card;     // on-list members of r
  bool taint;        // r has an off-list member
  bool early_taint;  // the early return left a set with an off-list member unvisited (diagnostics of the fixture)
};
// f(x) for every member of the intersection of the sets of classes [0, n)
template <class F>
KAMD_HD void aa_for_each_common(const SetTables& st, const AaClassList& cl, int n, F&& f) {
  if (n <= 0) return;
  int best = 0; uint64_t best_sz = ~0ULL;
  for (int j = 0; j < n; j++) { const uint32_t e = (uint32_t)cl.e[j * cl.stride]; const uint64_t sz = st.ec_off[e + 1] - st.ec_off[e]; if (sz < best_sz) { best_sz = sz; best = j; } }
  const uint32_t* base = st.ec_ids + st.ec_off[(uint32_t)cl.e[best * cl.stride]];
  for (uint64_t c = 0; c < best_sz; c++) {
    const uint32_t x = base[c];
    bool ok = true;
    for (int j = 0; ok && j < n; j++) {
      if (j == best) continue;
      const uint32_t e = (uint32_t)cl.e[j * cl.stride];
      const uint32_t* ids = st.ec_ids + st.ec_off[e];
      uint64_t lo = 0, hi = st.ec_off[e + 1] - st.ec_off[e];
      const uint64_t m = hi;
      while (lo < hi) { const uint64_t mid = (lo + hi) >> 1; if (ids[mid] < x) lo = mid + 1; else hi = mid; }
      ok = lo < m && ids[lo] == x;
    }
    if (ok) f(x);
  }
}
// onlist_bits (optional): also count the on-list members of a tainted r -- what the read rule WITHOUT its first step would
// look at; the product never asks for it
KAMD_HD AaFrameSet aa_frame_set(const SetTables& st, const uint8_t* ec_offlist, const AaClassList& cl, const uint32_t* onlist_bits = nullptr) {
  AaFrameSet fs{0u, false, false};
  int j = 0;
  while (j < cl.n && !ec_offlist[(uint32_t)cl.e[j * cl.stride]]) ++j;
  uint32_t card = 0;
  aa_for_each_common(st, cl, j, [&](uint32_t) { ++card; });
  if (j == cl.n) { fs.card = card; return fs; }
  if (j > 0 && card == 0) { fs.early_taint = true; return fs; }
  fs.taint = true;
  if (onlist_bits) aa_for_each_common(st, cl, cl.n, [&](uint32_t x) { if ((onlist_bits[x >> 5] >> (x & 31)) & 1u) ++fs.card; });
  return fs;
}

// ---------------------------------------------------------------------------------------------------------------
// intersectKmersCFC over the six frames' results, in frame order
// ---------------------------------------------------------------------------------------------------------------
enum { AA_ALIGNED = 0, AA_REJECT_OFFLIST = 1, AA_REJECT_EMPTY = 2 };
struct AaDecision { int outcome; int winner; uint32_t clashes; };
KAMD_HD AaDecision aa_read_rule(const uint32_t card[AA_FRAMES], uint32_t taint_mask) {
  AaDecision d{AA_REJECT_EMPTY, -1, 0u};
  if (taint_mask) { d.outcome = AA_REJECT_OFFLIST; return d; }                     // :53-64
  uint32_t smallest = 0xFFFFFFFFu;
  for (int f = 0; f < AA_FRAMES; f++) {                                            // :96-110
    if (card[f] > 0 && card[f] < smallest) { smallest = card[f]; d.winner = f; }
    else if (card[f] > 0 && card[f] == smallest) ++d.clashes;
  }
  if (d.winner >= 0) d.outcome = AA_ALIGNED;
  return d;
}

// the winner's distinct set ids, ascending (the order of a tuple record): sorts the list's low halves in place; returns their number
KAMD_HD int aa_classlist_to_sets(AaClassList& cl) {
  for (int i = 0; i < cl.n; i++) cl.e[i * cl.stride] &= 0xFFFFFFFFULL;
  for (int i = 1; i < cl.n; i++) {
    const uint64_t x = cl.e[i * cl.stride];
    int j = i;
    for (; j > 0 && cl.e[(j - 1) * cl.stride] > x; --j) cl.e[j * cl.stride] = cl.e[(j - 1) * cl.stride];
    cl.e[j * cl.stride] = x;
  }
  int m = 0;
  for (int i = 0; i < cl.n; i++)
    if (m == 0 || cl.e[(m - 1) * cl.stride] != cl.e[i * cl.stride]) cl.e[m++ * cl.stride] = cl.e[i * cl.stride];
  return m;
}

}  // namespace kamd
