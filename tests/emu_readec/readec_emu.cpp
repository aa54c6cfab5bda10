// tests/emu_readec/readec_emu.cpp -- TEST INFRASTRUCTURE: drives the table and the look-up of the per-read classes (kallisto_amd/csrc/kamd_readec.h)
// on the CPU, row by row and query by query, the way the kernels of kamd_readec.hip do thread by thread.  Never linked into libkallisto_amd.so.
#include "../../kallisto_amd/csrc/kamd_readec.h"

extern "C" {
uint64_t rec_emu_capacity(uint64_t n_ecs) { return kamd::rectable_capacity(n_ecs); }

// slots: 2 x cap words, zeroed here.  Returns the rows that found no slot (0 at any capacity >= the number of non-empty rows).
uint64_t rec_emu_build(const uint64_t* ec_off, const uint32_t* ec_ids, uint64_t n_ecs, uint64_t* slots, uint64_t cap, uint64_t tag_mask) {
  for (uint64_t i = 0; i < 2 * cap; i++) slots[i] = 0;
  const kamd::RecTable t{slots, cap, tag_mask};
  uint64_t failed = 0;
  for (uint64_t r = 0; r < n_ecs; r++)
    if (!kamd::rectable_insert_row(t, ec_off, ec_ids, r, [](uint64_t* p, uint64_t expect, uint64_t want) { const uint64_t old = *p; if (old == expect) *p = want; return old; }))
      ++failed;
  return failed;
}

// query q = q_ids[q_off[q] .. q_off[q + 1]) (ascending) -> out[q] = its row, KAMD_READ_EC_NONE or KAMD_READ_EC_FOREIGN
void rec_emu_lookup(const uint64_t* slots, uint64_t cap, uint64_t tag_mask, const uint64_t* ec_off, const uint32_t* ec_ids, const uint64_t* q_off,
                    const uint32_t* q_ids, uint64_t n_q, int32_t* out) {
  const kamd::RecTable t{const_cast<uint64_t*>(slots), cap, tag_mask};
  for (uint64_t q = 0; q < n_q; q++)
    out[q] = kamd::rectable_lookup(t, ec_off, ec_ids, [&](auto&& f) { for (uint64_t j = q_off[q]; j < q_off[q + 1]; j++) f(q_ids[j]); });
}
}
