// kamd_buscorrect.h -- barcode whitelists (`bustools correct`, restated): the membership table of kamd_bus_whitelist_create and the rule of
// kamd_bus_correct.  Host + device: kamd_buscorrect.hip runs them per record and per neighbour, tests/emu_buscorrect drives the same functions on
// the CPU.
//
//   whitelist   a set W of distinct barcodes of one length L (1 .. 32 bases), encoded as the records hold them: A0 C1 G2 T3, the first base most
//               significant, 2 L bits, all higher bits zero.
//   table       buckets of WL_BUCKET_KEYS = 8 keys (64 bytes: one line per probe).  A key's home bucket is wl_home; a key that finds its bucket full
//               goes on in the next one, wrapping at the end.  wl_n_buckets(n) = the power of two >= n / 4, at least 1: eight slots per bucket, so
//               at most half of the slots are taken and every walk ends at an empty slot.  Slots fill from the front of a bucket and are never
//               freed: the first empty slot of a walk ends it.
//   marker      an empty slot holds WL_EMPTY = 2^64 - 1.  For L < 32 that is no barcode (bits above 2 L).  At L = 32 it is 32 T: that barcode is never
//               stored, "it is in W" is the flag has_marker of the table, found on the host when the whitelist is created.
//   neighbour   j in [0, 3 L): position j / 3 (0 = the first base), the base there XOR (j % 3) + 1 -- the three other bases.
//   status      N(b) = the neighbours of b that are in W.  EXACT: b in W.  Else CORRECTED with |N(b)| = 1 (the barcode becomes that member),
//               AMBIGUOUS with |N(b)| >= 2, UNCORRECTABLE with |N(b)| = 0.  A barcode with a bit above 2 L - 1 is UNCORRECTABLE without a look-up.
#pragma once

#include <stdint.h>

#include "../../include/kallisto_amd.h"
#include "kamd_core.h"

namespace kamd {

constexpr int WL_BUCKET_KEYS = 8;
constexpr uint64_t WL_EMPTY = ~0ULL;

struct WlTable {
  const uint64_t* slots;   // n_buckets * WL_BUCKET_KEYS
  uint64_t n_buckets;      // a power of two
  int32_t bc_len;          // L
  int32_t has_marker;      // L = 32 only: WL_EMPTY itself is a member
};

KAMD_HD uint64_t wl_n_buckets(uint64_t n) {
  uint64_t b = 1;
  while (4 * b < n) b <<= 1;
  return b;
}
KAMD_HD uint64_t wl_home(uint64_t key, uint64_t n_buckets) { return mix64(key) & (n_buckets - 1); }
// the bits no barcode of L bases has
KAMD_HD uint64_t wl_high_mask(int L) { return L >= 32 ? 0ULL : ~0ULL << (2 * L); }
KAMD_HD uint64_t wl_neighbour(uint64_t b, int L, int j) { return b ^ ((uint64_t)(j % 3 + 1) << (2 * (L - 1 - j / 3))); }

// one bucket of a walk: 1 the key is there, -1 an empty slot and no key before it (the walk ends: not a member), 0 full of other keys (go on)
KAMD_HD int wl_bucket_scan(const uint64_t* k, uint64_t key) {
  int r = 0;
  for (int s = WL_BUCKET_KEYS - 1; s >= 0; s--) {   // (back to front: an empty slot has only empty slots behind it, the key lies before them)
    if (k[s] == WL_EMPTY) r = -1;
    if (k[s] == key) r = 1;
  }
  return r;
}

// load(bucket, k): the bucket's eight keys into k.  The table's load ends every walk; the trip count is bounded all the same
template <class Load>
KAMD_HD bool wl_contains_with(const WlTable& t, uint64_t key, Load&& load) {
  if (key == WL_EMPTY) return t.has_marker != 0;
  uint64_t b = wl_home(key, t.n_buckets);
  for (uint64_t trip = 0; trip < t.n_buckets; trip++) {
    uint64_t k[WL_BUCKET_KEYS];
    load(b, k);
    const int r = wl_bucket_scan(k, key);
    if (r) return r > 0;
    b = (b + 1) & (t.n_buckets - 1);
  }
  return false;
}
KAMD_HD bool wl_contains(const WlTable& t, uint64_t key) {
  return wl_contains_with(t, key, [&](uint64_t b, uint64_t* k) {
    for (int s = 0; s < WL_BUCKET_KEYS; s++) k[s] = t.slots[b * WL_BUCKET_KEYS + s];
  });
}

// the status of a miss from the number of its neighbours in W
KAMD_HD int wl_miss_status(uint32_t n_hits) {
  return n_hits == 1 ? KAMD_BUS_COR_CORRECTED : (n_hits >= 2 ? KAMD_BUS_COR_AMBIGUOUS : KAMD_BUS_COR_UNCORRECTABLE);
}

// a slot-claiming insertion, cas(p, expect, want) -> the value found: the first empty slot from the home bucket on, or the key itself (a duplicate).
// -> the buckets visited (1: the home bucket took it); *is_new: a slot was claimed.  0: no slot in n_buckets buckets (cannot happen at load <= 0.5)
template <class Cas>
KAMD_HD uint32_t wl_insert(uint64_t* slots, uint64_t n_buckets, uint64_t key, bool* is_new, Cas&& cas) {
  uint64_t b = wl_home(key, n_buckets);
  *is_new = false;
  for (uint64_t trip = 0; trip < n_buckets; trip++) {
    for (int s = 0; s < WL_BUCKET_KEYS; s++) {
      uint64_t* p = slots + b * WL_BUCKET_KEYS + s;
      uint64_t old = *p;   // (a slot goes from empty to its key once: a stale empty only means the compare-and-swap is taken after all)
      if (old == WL_EMPTY) old = cas(p, WL_EMPTY, key);
      if (old == WL_EMPTY) { *is_new = true; return (uint32_t)trip + 1; }
      if (old == key) return (uint32_t)trip + 1;
    }
    b = (b + 1) & (n_buckets - 1);
  }
  return 0;
}

// the rule for one barcode, the neighbours one after the other (the device gives every neighbour a lane instead): -> status, *fixed = the barcode
// the record keeps (EXACT, CORRECTED)
KAMD_HD int wl_correct_one(const WlTable& t, uint64_t b, uint64_t* fixed) {
  *fixed = b;
  if (b & wl_high_mask(t.bc_len)) return KAMD_BUS_COR_UNCORRECTABLE;
  if (wl_contains(t, b)) return KAMD_BUS_COR_EXACT;
  uint32_t hits = 0;
  for (int j = 0; j < 3 * t.bc_len; j++) {
    const uint64_t nb = wl_neighbour(b, t.bc_len, j);
    if (wl_contains(t, nb)) { ++hits; *fixed = nb; }
  }
  if (hits != 1) *fixed = b;
  return wl_miss_status(hits);
}

}  // namespace kamd
