// tests/emu_bustag/bustag_emu.cpp -- TEST INFRASTRUCTURE: drives the per-item rules of the barcode / UMI technologies (kallisto_amd/csrc/kamd_bustag.h)
// on the CPU, item by item in input order, the way the kernels of kamd_bus.hip do thread by thread; the layout parser (kamd_bus.cpp) is compiled in as
// it is.  Never linked into libkallisto_amd.so.
#include "../../kallisto_amd/csrc/kamd_bustag.h"

#include <cstring>

extern "C" {
int bus_emu_parse(const char* tech, kamd_bus_layout* out, int32_t* strand, char* err, size_t cap) { return kamd_bus_layout_parse(tech, out, strand, err, cap); }
int bus_emu_check(const kamd_bus_layout* L, char* err, size_t cap) { return kamd::bus_layout_check(L, err, cap); }
int32_t bus_emu_seq_max_len(const kamd_bus_layout* L, int32_t max_len) { return kamd_bus_seq_max_len(L, max_len); }
uint64_t bus_emu_record_words(int32_t max_len) { return (uint64_t)((max_len + 15) / 16 + 1) + (uint64_t)((max_len + 31) / 32 + 1); }

// the batch as kamd_bus_split takes it -> its outputs (only the first n_valid entries are written) and statistics; returns n_valid
uint64_t bus_emu_split(const kamd_bus_layout* L, const uint32_t* words, const uint16_t* lens, uint64_t n_items, int32_t max_len, kamd_bus_tag* tags, uint32_t* src,
                       uint32_t* seq_words, uint16_t* seq_len, int32_t seq_max_len, kamd_bus_split_stats* st) {
  memset(st, 0, sizeof *st);
  st->n_items = n_items;
  const int sw = (max_len + 15) / 16 + 1, rw = (int)bus_emu_record_words(max_len);
  const int osw = (seq_max_len + 15) / 16 + 1, orw = (int)bus_emu_record_words(seq_max_len);
  uint64_t j = 0;
  for (uint64_t i = 0; i < n_items; i++) {
    const int l0 = lens[i * L->n_files], l1 = L->n_files > 1 ? lens[i * L->n_files + 1] : 0;
    const kamd::BusLens ln = kamd::bus_item_lens(*L, l0, l1);
    if (ln.status != kamd::BUS_ITEM_DROP_UMI && kamd::bus_len_counted(ln.umi_len)) st->umi_len_hist[ln.umi_len]++;
    if (ln.status == kamd::BUS_ITEM_DROP_UMI) { st->n_dropped_umi++; continue; }
    if (ln.status == kamd::BUS_ITEM_DROP_BC) { st->n_dropped_bc++; continue; }
    if (kamd::bus_len_counted(ln.bc_len)) st->bc_len_hist[ln.bc_len]++;
    const uint32_t* rec = words + i * (uint64_t)L->n_files * rw;
    const kamd::BusItemView it{{rec, L->n_files > 1 ? rec + rw : rec}, {l0, l1}, sw};
    tags[j] = kamd::bus_item_tag(*L, it, ln);
    src[j] = (uint32_t)i;
    const int len = ln.seq_len < seq_max_len ? ln.seq_len : seq_max_len;
    seq_len[j] = (uint16_t)len;
    if (len > st->max_seq_len) st->max_seq_len = len;
    const uint32_t* srec = rec + (uint64_t)L->seq.file * rw;
    uint32_t* out = seq_words + j * (uint64_t)orw;
    uint32_t any = 0;
    for (int w = 0; w < orw - osw; w++) any |= (out[osw + w] = kamd::bus_cut_mask_word(srec + sw, rw - sw, ln.seq_start, len, w));
    for (int w = 0; w < osw - 1; w++) out[w] = kamd::bus_cut_seq_word(srec, sw, ln.seq_start, len, w);
    out[osw - 1] = any ? kamd::REC_FLAG_HAS_N : 0u;
    ++j;
  }
  st->n_valid = j;
  return j;
}
}
