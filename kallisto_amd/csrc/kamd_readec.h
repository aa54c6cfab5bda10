// kamd_readec.h -- per-read equivalence classes: the look-up of an item's transcript set in a finalized EC result (kamd_read_ecs).  Host + device:
// kamd_readec.hip runs it one item per thread, tests/emu_readec drives the same functions on the CPU.
//
//   the table   one 16-byte slot {tag, row} per class of the result, open addressing with linear probing, capacity a power of two >= 2 x n_ecs.
//               tag = hash of the row's sorted ids (the chained mix64 form of rec_hash with the length folded in at the end, so that it can be
//               computed while a set is being enumerated, before its size is known); 0 marks an empty slot.  A slot is claimed with one 64-bit
//               compare-and-swap on its tag; the row is written by the claimant and read only by later launches.
//   the look-up the set is never stored: it is enumerated once for its size and tag, and once more against ec_ids[ec_off[row] ..] of every
//               probed slot whose tag and size match.  A tag match with other members continues the probe; an empty slot ends it (FOREIGN);
//               a probe visits every slot at most once.
#pragma once

#include <stdint.h>

#include "../../include/kallisto_amd.h"
#include "kamd_core.h"

namespace kamd {

struct SetHash { uint64_t h; uint32_t n; };
KAMD_HD void sethash_init(SetHash& s) { s.h = 0x9e3779b97f4a7c15ULL; s.n = 0; }
KAMD_HD void sethash_add(SetHash& s, uint32_t x) { s.h = mix64(s.h ^ x); ++s.n; }
// tag_mask: ~0 in the product; the tests pass 0 (every tag equal: the member compare and the continued probe decide alone)
KAMD_HD uint64_t sethash_tag(const SetHash& s, uint64_t tag_mask) { return (mix64(s.h ^ (0xc2b2ae3d27d4eb4fULL * (s.n + 1))) & tag_mask) | 1ULL; }

struct RecTable {
  uint64_t* slots;     // 2 x cap words: {tag, row}
  uint64_t cap;        // power of two
  uint64_t tag_mask;
};
KAMD_HD uint64_t rectable_capacity(uint64_t n_ecs) {   // the smallest power of two >= 2 x n_ecs (and >= 2)
  uint64_t c = 2;
  while (c < 2 * n_ecs) c <<= 1;
  return c;
}
KAMD_HD uint64_t rectable_home(const RecTable& t, uint64_t tag) { return (tag >> 20) & (t.cap - 1); }

// cas(p, expected, desired) -> the old value of *p.  false: no free slot (cannot happen at the capacity above)
template <class Cas>
KAMD_HD bool rectable_insert(const RecTable& t, uint64_t tag, uint64_t row, Cas&& cas) {
  uint64_t s = rectable_home(t, tag);
  for (uint64_t probe = 0; probe < t.cap; probe++, s = (s + 1) & (t.cap - 1))
    if (cas(&t.slots[2 * s], 0ULL, tag) == 0ULL) { t.slots[2 * s + 1] = row; return true; }
  return false;
}
// row r of the CSR -> the table (an empty row is not a class: skipped)
template <class Cas>
KAMD_HD bool rectable_insert_row(const RecTable& t, const uint64_t* ec_off, const uint32_t* ec_ids, uint64_t r, Cas&& cas) {
  SetHash sh; sethash_init(sh);
  for (uint64_t j = ec_off[r]; j < ec_off[r + 1]; j++) sethash_add(sh, ec_ids[j]);
  if (sh.n == 0) return true;
  return rectable_insert(t, sethash_tag(sh, t.tag_mask), r, cas);
}

// en(f): calls f(x) for every member of the item's set, ascending, the same sequence every time it is called
template <class Enum>
KAMD_HD int32_t rectable_lookup(const RecTable& t, const uint64_t* ec_off, const uint32_t* ec_ids, Enum&& en) {
  SetHash sh; sethash_init(sh);
  en([&](uint32_t x) { sethash_add(sh, x); });
  if (sh.n == 0) return KAMD_READ_EC_NONE;
  const uint64_t tag = sethash_tag(sh, t.tag_mask);
  uint64_t s = rectable_home(t, tag);
  for (uint64_t probe = 0; probe < t.cap; probe++, s = (s + 1) & (t.cap - 1)) {
    const uint64_t st = t.slots[2 * s];
    if (st == 0) return KAMD_READ_EC_FOREIGN;
    if (st != tag) continue;
    const uint64_t row = t.slots[2 * s + 1], off = ec_off[row];
    if (ec_off[row + 1] - off != sh.n) continue;
    bool same = true; uint32_t j = 0;
    en([&](uint32_t x) { if (j < sh.n) same = same && ec_ids[off + j] == x; ++j; });
    if (same && j == sh.n) return (int32_t)row;
  }
  return KAMD_READ_EC_FOREIGN;
}

}  // namespace kamd
