// tests/emu_buscorrect/buscorrect_emu.cpp -- TEST INFRASTRUCTURE: drives the whitelist table and the correction rule of kamd_bus_whitelist_create /
// kamd_bus_correct (kallisto_amd/csrc/kamd_buscorrect.h) on the CPU: a plain host build of the table, key by key in input order, the look-up, and the
// rule over an array of records.  Never linked into libkallisto_amd.so.
#include "../../kallisto_amd/csrc/kamd_buscorrect.h"

#include <cstring>
#include <vector>

struct EmuWhitelist {
  std::vector<uint64_t> slots;
  kamd::WlTable t;
  uint64_t n_distinct;
  uint32_t max_chain;
};

extern "C" {
uint64_t buscorrect_emu_n_buckets(uint64_t n) { return kamd::wl_n_buckets(n); }
uint64_t buscorrect_emu_home(uint64_t key, uint64_t n_buckets) { return kamd::wl_home(key, n_buckets); }
uint64_t buscorrect_emu_neighbour(uint64_t b, int L, int j) { return kamd::wl_neighbour(b, L, j); }

// the table of codes[0 .. n) with n_buckets buckets (0: the capacity rule's); NULL: a code with high bits, no codes, a length outside 1 .. 32, or
// n_buckets no power of two or too small for load <= 1
EmuWhitelist* buscorrect_emu_build(const uint64_t* codes, uint64_t n, int32_t bc_len, uint64_t n_buckets) {
  if (n == 0 || bc_len < 1 || bc_len > 32) return nullptr;
  if (n_buckets == 0) n_buckets = kamd::wl_n_buckets(n);
  if ((n_buckets & (n_buckets - 1)) || n_buckets * kamd::WL_BUCKET_KEYS <= n) return nullptr;
  for (uint64_t i = 0; i < n; i++)
    if (codes[i] & kamd::wl_high_mask(bc_len)) return nullptr;
  EmuWhitelist* w = new EmuWhitelist;
  w->slots.assign(n_buckets * kamd::WL_BUCKET_KEYS, kamd::WL_EMPTY);
  w->n_distinct = 0; w->max_chain = 0;
  int32_t has_marker = 0;
  for (uint64_t i = 0; i < n; i++) {
    if (codes[i] == kamd::WL_EMPTY) { has_marker = 1; continue; }
    bool is_new = false;
    const uint32_t chain = kamd::wl_insert(w->slots.data(), n_buckets, codes[i], &is_new, [](uint64_t* p, uint64_t expect, uint64_t want) {
      const uint64_t old = *p;
      if (old == expect) *p = want;
      return old;
    });
    if (chain == 0) { delete w; return nullptr; }
    if (is_new) ++w->n_distinct;
    if (chain > w->max_chain) w->max_chain = chain;
  }
  w->n_distinct += (uint64_t)has_marker;
  w->t = kamd::WlTable{w->slots.data(), n_buckets, bc_len, has_marker};
  return w;
}
void buscorrect_emu_free(EmuWhitelist* w) { delete w; }
uint64_t buscorrect_emu_distinct(const EmuWhitelist* w) { return w->n_distinct; }
uint32_t buscorrect_emu_max_chain(const EmuWhitelist* w) { return w->max_chain; }
uint64_t buscorrect_emu_table_buckets(const EmuWhitelist* w) { return w->t.n_buckets; }
int buscorrect_emu_lookup(const EmuWhitelist* w, uint64_t key) { return kamd::wl_contains(w->t, key) ? 1 : 0; }

// in[0 .. n) -> out (the survivors, compact, in order), status[0 .. n) (nullable), counts[4] by status; returns the survivors
uint64_t buscorrect_emu_correct(const EmuWhitelist* w, const kamd_bus_record* in, uint64_t n, kamd_bus_record* out, uint8_t* status, uint64_t* counts) {
  uint64_t m = 0;
  memset(counts, 0, 4 * sizeof *counts);
  for (uint64_t i = 0; i < n; i++) {
    uint64_t fixed = 0;
    const int s = kamd::wl_correct_one(w->t, in[i].barcode, &fixed);
    if (status) status[i] = (uint8_t)s;
    ++counts[s];
    if (s <= KAMD_BUS_COR_CORRECTED) { out[m] = in[i]; out[m].barcode = fixed; ++m; }
  }
  return m;
}
}
