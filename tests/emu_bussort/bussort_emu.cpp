// tests/emu_bussort/bussort_emu.cpp -- TEST INFRASTRUCTURE: drives the per-record rules of kamd_bus_sort / kamd_bus_count
// (kallisto_amd/csrc/kamd_bussort.h) on the CPU, record by record in input order: a plain LSD sort over bus_key_digit with the passes bus_sort_plan
// names, the collapse, and the rows / groups / multi-class rule of the count.  Never linked into libkallisto_amd.so.
#include "../../kallisto_amd/csrc/kamd_bussort.h"

#include <cstring>
#include <vector>

extern "C" {
uint32_t bussort_emu_digit(const kamd_bus_record* r, int d) { return kamd::bus_key_digit(*r, d); }
uint32_t bussort_emu_plan(const uint8_t* or_bits, const uint8_t* and_bits) { return kamd::bus_sort_plan(or_bits, and_bits); }

// OR and AND of the keys of rec[0 .. n), digit by digit (or_bits / and_bits: BUS_KEY_DIGITS bytes each) -> the plan
uint32_t bussort_emu_reduce(const kamd_bus_record* rec, uint64_t n, uint8_t* or_bits, uint8_t* and_bits) {
  memset(or_bits, 0, kamd::BUS_KEY_DIGITS);
  memset(and_bits, n ? 0xFF : 0, kamd::BUS_KEY_DIGITS);   // (no records: no digit differs)
  for (uint64_t i = 0; i < n; i++)
    for (int d = 0; d < kamd::BUS_KEY_DIGITS; d++) {
      const uint8_t x = (uint8_t)kamd::bus_key_digit(rec[i], d);
      or_bits[d] |= x; and_bits[d] &= x;
    }
  return kamd::bus_sort_plan(or_bits, and_bits);
}

// stable LSD sort of rec[0 .. n) in place: one counting pass per digit of the plan; returns the plan
uint32_t bussort_emu_sort(kamd_bus_record* rec, uint64_t n) {
  uint8_t o[kamd::BUS_KEY_DIGITS], a[kamd::BUS_KEY_DIGITS];
  const uint32_t plan = bussort_emu_reduce(rec, n, o, a);
  std::vector<kamd_bus_record> tmp(n);
  kamd_bus_record *src = rec, *dst = tmp.data();
  for (int d = 0; d < kamd::BUS_KEY_DIGITS; d++) {
    if (!((plan >> d) & 1u)) continue;
    uint64_t start[257] = {0};
    for (uint64_t i = 0; i < n; i++) start[kamd::bus_key_digit(src[i], d) + 1]++;
    for (int x = 0; x < 256; x++) start[x + 1] += start[x];
    for (uint64_t i = 0; i < n; i++) dst[start[kamd::bus_key_digit(src[i], d)]++] = src[i];
    kamd_bus_record* t = src; src = dst; dst = t;
  }
  if (src != rec) memcpy(rec, src, n * sizeof *rec);
  return plan;
}

// runs of equal keys -> one record, count summed in 64 bits, pad of the first; in place; *n_over: runs whose sum exceeds 32 bits (count left as it was)
uint64_t bussort_emu_collapse(kamd_bus_record* rec, uint64_t n, uint64_t* n_over) {
  uint64_t j = 0;
  *n_over = 0;
  for (uint64_t i = 0; i < n;) {
    uint64_t e = i, sum = 0;
    while (e < n && kamd::bus_key_equal(rec[i], rec[e])) sum += rec[e++].count;
    kamd_bus_record r = rec[i];
    if (sum > 0xFFFFFFFFULL) ++*n_over; else r.count = (uint32_t)sum;
    rec[j++] = r;
    i = e;
  }
  return j;
}

// pairs of neighbours out of key order
uint64_t bussort_emu_unsorted(const kamd_bus_record* rec, uint64_t n) {
  uint64_t k = 0;
  for (uint64_t i = 1; i < n; i++) k += kamd::bus_key_less(rec[i], rec[i - 1]) ? 1 : 0;
  return k;
}

// kamd_bus_count on records in key order: barcodes [n], entries [n], multi [n]; stats as kamd_bus_count_stats; returns the number of sums above 32 bits
uint64_t bussort_emu_count(const kamd_bus_record* rec, uint64_t n, int mode, uint64_t* barcodes, kamd_bus_entry* entries, kamd_bus_record* multi,
                           kamd_bus_count_stats* st) {
  memset(st, 0, sizeof *st);
  st->n_records = n;
  std::vector<kamd_bus_record> units;
  uint64_t row = 0;
  for (uint64_t i = 0; i < n;) {
    if (i == 0 || !kamd::bus_same_barcode(rec[i - 1], rec[i])) { barcodes[st->n_barcodes++] = rec[i].barcode; row = st->n_barcodes - 1; }
    uint64_t e = i + 1;
    while (e < n && kamd::bus_same_group(rec[i], rec[e])) ++e;
    st->n_umis++;
    if (mode == KAMD_BUS_COUNT_READS) {
      for (uint64_t k = i; k < e; k++) units.push_back(kamd::bus_unit_record(rec[k], (uint32_t)row, mode));
    } else if (kamd::bus_group_multi(rec[i], rec[e - 1])) {
      st->n_multi_groups++;
      for (uint64_t k = i; k < e; k++) { multi[st->n_multi_records] = rec[k]; multi[st->n_multi_records++].pad = (uint32_t)row; }
    } else {
      units.push_back(kamd::bus_unit_record(rec[i], (uint32_t)row, mode));
    }
    i = e;
  }
  uint64_t n_over = 0;
  bussort_emu_sort(units.data(), units.size());
  const uint64_t m = bussort_emu_collapse(units.data(), units.size(), &n_over);
  for (uint64_t j = 0; j < m; j++) { entries[j].row = units[j].pad; entries[j].ec = units[j].ec; entries[j].value = units[j].count; }
  st->n_entries = m;
  return n_over;
}
}
