// kamd_busgenes.h -- BUS records to a cells x genes matrix (`bustools count --genecounts -g t2g.txt`, restated): the gene lists of the classes and
// the rule that gives a group of records its gene.  Host + device: kamd_busgenes.hip runs them per group, tests/emu_busgenes drives the same
// functions on the CPU.
//
//   gene map    every transcript has a gene id in [0, n_genes), or -1: no gene.
//   gene list   G(c) of a class c: the sorted, distinct gene ids (>= 0) of c's transcripts; a transcript without a gene adds nothing, G(c) may be
//               empty.  The lists of all classes are a CSR: off[n_classes + 1], ids.  They are built from one key {barcode = class, umi = gene}
//               per entry of the classes' CSR whose transcript has a gene: kamd_bus_sort's order and collapse leave the distinct pairs sorted.
//   group       UMIS: a run of equal (barcode, umi), as kamd_bus_count's; READS: every record by itself.
//   rule        I = the intersection of G(c) over the group's records.  |I| = 1: the group counts for that gene (UMIS: 1, READS: the record's
//               count); |I| = 0: GENE_NONE; |I| >= 2: GENE_MULTI; both are dropped.  A class that the group names twice changes nothing.
//   candidates  I is a subset of every list, so the members of the group's smallest list (the first record wins a tie) are tried one by one
//               against the lists of the other records; the trial ends at the second survivor.
//   who settles a thread settles a group of one record (the length of its list and the list's first id) and a group of at most
//               GENES_THREAD_MAX_RECORDS records whose smallest list has at most GENES_THREAD_MAX_LIST genes; a wavefront settles every other group.
#pragma once

#include <stdint.h>

#include "../../include/kallisto_amd.h"
#include "kamd_core.h"

namespace kamd {

constexpr uint32_t GENES_THREAD_MAX_RECORDS = 4;   // (both are choices that nobody has measured: DESIGN.md section 6i)
constexpr uint32_t GENES_THREAD_MAX_LIST = 8;
constexpr int32_t GENE_NONE = -1, GENE_MULTI = -2;

struct GeneLists { const uint64_t* off; const int32_t* ids; uint64_t n_classes; };

KAMD_HD bool gene_class_ok(const GeneLists& t, int32_t c) { return c >= 0 && (uint64_t)c < t.n_classes; }
KAMD_HD uint32_t gene_list_len(const GeneLists& t, int32_t c) { return (uint32_t)(t.off[c + 1] - t.off[c]); }
KAMD_HD bool gene_list_has(const GeneLists& t, int32_t c, int32_t x) {
  const int32_t* ids = t.ids + t.off[c];
  uint32_t lo = 0, hi = gene_list_len(t, c);
  const uint32_t n = hi;
  while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if (ids[mid] < x) lo = mid + 1; else hi = mid; }
  return lo < n && ids[lo] == x;
}
// the gene of a group of one record
KAMD_HD int32_t gene_of_class(const GeneLists& t, int32_t c) {
  const uint32_t len = gene_list_len(t, c);
  return len == 1 ? t.ids[t.off[c]] : (len == 0 ? GENE_NONE : GENE_MULTI);
}
// does a thread settle a group of m records whose smallest list has min_len genes
KAMD_HD bool gene_group_small(uint64_t m, uint32_t min_len) { return m <= 1 || (m <= GENES_THREAD_MAX_RECORDS && min_len <= GENES_THREAD_MAX_LIST); }

// the record of a group of m records with the smallest list, the first of equals; class_at(k) = the class of record k, each in range
template <class ClassAt>
KAMD_HD uint64_t gene_group_pivot(const GeneLists& t, uint64_t m, ClassAt&& class_at, uint32_t* min_len) {
  uint64_t best = 0;
  uint32_t len = gene_list_len(t, class_at(0));
  for (uint64_t k = 1; k < m; k++) {
    const uint32_t l = gene_list_len(t, class_at(k));
    if (l < len) { len = l; best = k; }
  }
  *min_len = len;
  return best;
}
// the rule, serially: every candidate of the pivot's list against the lists of the other records
template <class ClassAt>
KAMD_HD int32_t gene_of_group(const GeneLists& t, uint64_t m, ClassAt&& class_at) {
  uint32_t len = 0;
  const uint64_t pivot = gene_group_pivot(t, m, class_at, &len);
  const int32_t* cand = t.ids + t.off[class_at(pivot)];
  uint32_t survivors = 0;
  int32_t gene = GENE_NONE;
  for (uint32_t j = 0; j < len && survivors < 2; j++) {
    bool in_all = true;
    for (uint64_t k = 0; k < m && in_all; k++)
      if (k != pivot) in_all = gene_list_has(t, class_at(k), cand[j]);
    if (in_all) { ++survivors; gene = cand[j]; }
  }
  return survivors == 1 ? gene : (survivors == 0 ? GENE_NONE : GENE_MULTI);
}

// the key of a (class, gene) pair as a record that kamd_bus_sort takes
KAMD_HD kamd_bus_record gene_pair_record(uint64_t cls, int32_t gene) {
  kamd_bus_record r;
  r.barcode = cls; r.umi = (uint64_t)(uint32_t)gene; r.ec = 0; r.count = 1u; r.flags = 0; r.pad = 0;
  return r;
}
// the class of entry i of a CSR: the c with off[c] <= i < off[c + 1] (classes without entries are passed over); i below off[n_classes]
KAMD_HD uint64_t csr_row_of(const uint64_t* off, uint64_t n_classes, uint64_t i) {
  uint64_t lo = 0, hi = n_classes;   // the first c with off[c + 1] > i
  while (lo < hi) { const uint64_t mid = (lo + hi) >> 1; if (off[mid + 1] <= i) lo = mid + 1; else hi = mid; }
  return lo;
}

}  // namespace kamd
