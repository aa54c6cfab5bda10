// kamd_bussort.h -- BUS records to a cells x classes matrix (`bustools sort | bustools count`, restated): the per-item rules of kamd_bus_sort and
// kamd_bus_count.  Host + device: kamd_bussort.hip runs them per record, tests/emu_bussort drives the same functions on the CPU.
//
//   key         a record's sort key, most significant first: barcode (u64), umi (u64), ec (signed: its top bit is flipped when digits are taken),
//               flags (u32) -- the order of np.lexsort((flags, ec, umi, barcode)).  8 + 8 + 4 + 4 = 24 bytes, so 24 digits of 8 bits: digit 0 is
//               the least significant byte of flags, digit 23 the most significant byte of barcode.  `count` and `pad` are no part of the key.
//   plan        an LSD pass is needed only for a digit in which two keys differ: OR and AND of the keys are reduced once, a digit whose OR byte
//               equals its AND byte is the same in every key and is skipped.
//   collapse    records equal in all four key fields become one, count = the sum (held in 64 bits, above 0xFFFFFFFF is an error), pad of the first.
//   rows        (kamd_bus_count) the distinct barcodes, ascending.
//   group       a run of equal (barcode, umi), flags ignored.  Inside a group the records are in ec order, so the group names several classes
//               exactly when its first and its last record differ in ec.  A group of one class counts 1 for (row, class); a group of several
//               counts nothing and is handed to the host.
#pragma once

#include <stdint.h>

#include "../../include/kallisto_amd.h"
#include "kamd_core.h"

namespace kamd {

constexpr int BUS_KEY_DIGITS = 24;
constexpr int BUS_KEY_WORDS = 6;

// word w of the key as a little-endian number of 192 bits: flags, ec (top bit flipped), umi low / high, barcode low / high
KAMD_HD uint32_t bus_key_word(const kamd_bus_record& r, int w) {
  switch (w) {
    case 0: return r.flags;
    case 1: return (uint32_t)r.ec ^ 0x80000000u;
    case 2: return (uint32_t)r.umi;
    case 3: return (uint32_t)(r.umi >> 32);
    case 4: return (uint32_t)r.barcode;
    default: return (uint32_t)(r.barcode >> 32);
  }
}
KAMD_HD uint32_t bus_key_digit(const kamd_bus_record& r, int d) { return (bus_key_word(r, d >> 2) >> (8 * (d & 3))) & 0xFFu; }

// or_bits / and_bits: digit d of the OR / the AND of all keys -> bit d set: an LSD pass over digit d is needed
KAMD_HD uint32_t bus_sort_plan(const uint8_t* or_bits, const uint8_t* and_bits) {
  uint32_t m = 0;
  for (int d = 0; d < BUS_KEY_DIGITS; d++)
    if (or_bits[d] != and_bits[d]) m |= 1u << d;
  return m;
}

KAMD_HD bool bus_key_equal(const kamd_bus_record& a, const kamd_bus_record& b) {
  return a.barcode == b.barcode && a.umi == b.umi && a.ec == b.ec && a.flags == b.flags;
}
// a before b in key order
KAMD_HD bool bus_key_less(const kamd_bus_record& a, const kamd_bus_record& b) {
  if (a.barcode != b.barcode) return a.barcode < b.barcode;
  if (a.umi != b.umi) return a.umi < b.umi;
  if (a.ec != b.ec) return a.ec < b.ec;
  return a.flags < b.flags;
}
KAMD_HD bool bus_same_barcode(const kamd_bus_record& a, const kamd_bus_record& b) { return a.barcode == b.barcode; }
KAMD_HD bool bus_same_group(const kamd_bus_record& a, const kamd_bus_record& b) { return a.barcode == b.barcode && a.umi == b.umi; }
// first / last: the first and the last record of a group of records in key order
KAMD_HD bool bus_group_multi(const kamd_bus_record& first, const kamd_bus_record& last) { return first.ec != last.ec; }

// what a counted group (KAMD_BUS_COUNT_UMIS: its first record) or a record (KAMD_BUS_COUNT_READS) adds to the matrix, as a record that
// kamd_bus_sort takes: the row in the barcode's place (rows ascend with the barcodes; fewer digits differ) and in pad, no UMI, no flags
KAMD_HD kamd_bus_record bus_unit_record(const kamd_bus_record& r, uint32_t row, int mode) {
  kamd_bus_record u;
  u.barcode = row; u.umi = 0; u.ec = r.ec; u.count = mode == KAMD_BUS_COUNT_READS ? r.count : 1u; u.flags = 0; u.pad = row;
  return u;
}

}  // namespace kamd
