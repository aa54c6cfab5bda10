// tests/emu_tupletag/tupletag_emu.cpp -- TEST INFRASTRUCTURE: the tag word of a tuple record in the table of distinct tuples (kamd_core.h tuple_tag, the
// one function every kernel that touches the table calls) on the CPU.  Never linked into libkallisto_amd.so.
#include "../../kallisto_amd/csrc/kamd_core.h"

// rec = [m, e0 ..].  *start: where the probe sequence begins; *is_short: the exact form
extern "C" uint64_t emu_tuple_tag(const uint32_t* rec, uint32_t short_id_bits, uint64_t* start, int32_t* is_short) {
  const kamd::TupleTag t = kamd::tuple_tag(rec, short_id_bits);
  if (start) *start = t.start;
  if (is_short) *is_short = t.is_short ? 1 : 0;
  return t.word;
}
// the record an exact tag names
extern "C" uint32_t emu_tuple_of_tag(uint64_t word, uint32_t short_id_bits, uint32_t* ids) { return kamd::tuple_of_tag(word, short_id_bits, ids); }
