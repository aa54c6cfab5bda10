// tests/emu_busgenes/busgenes_emu.cpp -- TEST INFRASTRUCTURE: drives the rules of kamd_bus_genes_create / kamd_bus_count_genes
// (kallisto_amd/csrc/kamd_busgenes.h) on the CPU: the gene lists from one key per entry with a gene, in kamd_bus_sort's order and collapsed; the
// rule of a group, group by group in input order; the two thresholds and which groups they hand to a wavefront.  Never linked into
// libkallisto_amd.so.
#include "../../kallisto_amd/csrc/kamd_busgenes.h"
#include "../../kallisto_amd/csrc/kamd_bussort.h"

#include <algorithm>
#include <cstring>
#include <map>
#include <utility>
#include <vector>

extern "C" {
void busgenes_emu_thresholds(uint32_t* max_records, uint32_t* max_list) { *max_records = kamd::GENES_THREAD_MAX_RECORDS; *max_list = kamd::GENES_THREAD_MAX_LIST; }

// the gene lists of the classes: out_off [n_classes + 1], out_ids [cap]; returns the number of distinct (class, gene) pairs (nothing beyond cap is written)
uint64_t busgenes_emu_lists(const int32_t* tr_gene, const uint64_t* ec_off, const uint32_t* ec_ids, uint64_t n_classes, uint64_t* out_off, int32_t* out_ids, uint64_t cap) {
  std::vector<kamd_bus_record> keys;
  for (uint64_t i = 0; i < ec_off[n_classes]; i++) {
    const int32_t g = tr_gene[ec_ids[i]];
    if (g >= 0) keys.push_back(kamd::gene_pair_record(kamd::csr_row_of(ec_off, n_classes, i), g));
  }
  std::stable_sort(keys.begin(), keys.end(), [](const kamd_bus_record& a, const kamd_bus_record& b) { return kamd::bus_key_less(a, b); });
  uint64_t n_pairs = 0;
  for (uint64_t c = 0; c <= n_classes; c++) out_off[c] = 0;
  for (size_t j = 0; j < keys.size(); j++) {
    if (j && kamd::bus_key_equal(keys[j - 1], keys[j])) continue;
    if (n_pairs < cap) out_ids[n_pairs] = (int32_t)(uint32_t)keys[j].umi;
    ++n_pairs;
    out_off[keys[j].barcode + 1]++;
  }
  for (uint64_t c = 0; c < n_classes; c++) out_off[c + 1] += out_off[c];
  return n_pairs;
}

// the gene of one group of m records (their classes, each in range), by the serial rule
int32_t busgenes_emu_group(const uint64_t* off, const int32_t* ids, uint64_t n_classes, const int32_t* classes, uint64_t m) {
  const kamd::GeneLists t{off, ids, n_classes};
  if (m == 1) return kamd::gene_of_class(t, classes[0]);
  return kamd::gene_of_group(t, m, [&](uint64_t k) { return classes[k]; });
}

// kamd_bus_count_genes on records in key order: barcodes [n], entries [n]; 0, or what ends the call with -4: 1 a class outside the table, 2 unsorted
// input, 3 a value above 32 bits (nothing is written then)
int busgenes_emu_count(const uint64_t* off, const int32_t* ids, uint64_t n_classes, const kamd_bus_record* rec, uint64_t n, int mode, uint64_t* barcodes,
                       kamd_bus_entry* entries, kamd_bus_gene_count_stats* st) {
  const kamd::GeneLists t{off, ids, n_classes};
  memset(st, 0, sizeof *st);
  for (uint64_t i = 1; i < n; i++) if (kamd::bus_key_less(rec[i], rec[i - 1])) return 2;
  for (uint64_t i = 0; i < n; i++) if (!kamd::gene_class_ok(t, rec[i].ec)) return 1;
  kamd_bus_gene_count_stats s;
  memset(&s, 0, sizeof s);
  s.n_records = n;
  std::vector<uint64_t> rows;
  std::map<std::pair<uint32_t, int32_t>, uint64_t> m;
  for (uint64_t i = 0; i < n;) {
    if (i == 0 || !kamd::bus_same_barcode(rec[i - 1], rec[i])) rows.push_back(rec[i].barcode);
    uint64_t e = i + 1;
    if (mode == KAMD_BUS_COUNT_UMIS) while (e < n && kamd::bus_same_group(rec[i], rec[e])) ++e;
    auto class_at = [&](uint64_t k) { return rec[i + k].ec; };
    const uint64_t len = e - i;
    int32_t gene;
    if (len == 1) gene = kamd::gene_of_class(t, rec[i].ec);
    else {
      uint32_t min_len = 0;
      kamd::gene_group_pivot(t, len, class_at, &min_len);
      if (!kamd::gene_group_small(len, min_len)) s.n_wave_groups++;
      gene = kamd::gene_of_group(t, len, class_at);
    }
    s.n_umis++;
    if (gene >= 0) {
      s.n_counted++;
      m[{(uint32_t)(rows.size() - 1), gene}] += kamd::bus_unit_record(rec[i], 0, mode).count;
    } else if (gene == kamd::GENE_NONE) s.n_no_gene++;
    else s.n_multi_gene++;
    i = e;
  }
  for (const auto& kv : m) if (kv.second > 0xFFFFFFFFULL) return 3;
  uint64_t j = 0;
  for (const auto& kv : m) { entries[j].row = kv.first.first; entries[j].ec = kv.first.second; entries[j].value = (uint32_t)kv.second; ++j; }
  for (size_t r = 0; r < rows.size(); r++) barcodes[r] = rows[r];
  s.n_barcodes = rows.size(); s.n_entries = j;
  *st = s;
  return 0;
}
}
