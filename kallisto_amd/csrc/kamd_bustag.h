// kamd_bustag.h -- barcode / UMI technologies (`bus -x <technology>`): what BUSProcessor::processBuffer does with one item in front of match()
// (src/ProcessReads.cpp:1486-1627) and for its record behind it (:1739-1746), for a layout without tag sequence, --paired, --batch-barcodes and
// batch mode.  Host + device: kamd_bus.hip runs it per item, tests/emu_bustag drives the same functions on the CPU.
//
//   an item     n_files consecutive packed records of one batch (all at the batch's max_len), as the FASTQ packers emit them.
//   a field     (barcode, UMI) up to KAMD_BUS_MAX_PARTS substrings (file, start, stop), concatenated; stop == 0: to the end of the read; file == -1 on
//               the first part: the field is absent.  A part that does not lie inside its read (l < start + len) or is empty DROPS the item: the
//               reference `continue`s before numreads++, such a read is not "processed".
//   encoding    stringToBinary (src/BUSData.cpp:8-36) over the first min(len, 32) bases of the concatenation: A0 C1 G2 T3, r = r << 2 | code; a base the
//               record's mask marks as not ACGT takes code 2 and counts as an N; flag = min(numN, 3) | (index of the first N & 31) << 2, 0 without N.
//               (A packed record only knows "ACGT or not": an IUPAC letter other than N is an N here; the reference's code for it follows the character's bits.)
//   absent      UMI: ~0, length 1 in the histogram, and the UMI half of the record's flags repeats the BARCODE's flag -- `f` still holds what
//               stringToBinary(bc) left in it when :1745 shifts it in (tests/golden/bus_sc/no_umi shows it).  Barcode: 0, length 16.
//   sequence    bases [start, stop ? stop : l) of the sequence part's read, clamped to the read; l <= start: an empty read that is processed and not
//               pseudoaligned.  (The reference passes match() the unclamped length, which reads past the string: identical whenever l >= max(start + 1, stop).)
//   repacking   word w of the cut's 2-bit half = source bases start + 16w ..., shifted across the source's word boundary; likewise the mask words in
//               steps of 32; everything at and beyond the cut's length is zero, the flag word says whether the cut holds an N: exactly what
//               kamd_pack_reads_host writes for the substring.
#pragma once

#include <stdint.h>

#include "../../include/kallisto_amd.h"
#include "kamd_core.h"

namespace kamd {

enum { BUS_ITEM_OK = 0, BUS_ITEM_DROP_UMI = 1, BUS_ITEM_DROP_BC = 2 };

struct BusLens { int status, bc_len, umi_len, seq_start, seq_len; };
struct BusItemView { const uint32_t* rec[2]; int len[2]; int seq_words; };   // seq_words: 2-bit words of a record incl. the flag word (the mask words follow)

KAMD_HD bool bus_field_absent(const kamd_bus_substr* parts) { return parts[0].file < 0; }

// total length of a present field, false = the item is dropped
KAMD_HD bool bus_field_len(const kamd_bus_substr* parts, int n, int l0, int l1, int* total) {
  int t = 0;
  for (int p = 0; p < n; p++) {
    const int l = parts[p].file ? l1 : l0;
    const int len = parts[p].stop ? parts[p].stop - parts[p].start : l - parts[p].start;
    if (l < parts[p].start + len || len <= 0) return false;
    t += len;
  }
  *total = t;
  return true;
}

// what the lengths of an item's reads decide: dropped or not (the UMI is looked at first, :1505-1521 before :1585-1602), the fields' lengths, the cut
KAMD_HD BusLens bus_item_lens(const kamd_bus_layout& L, int l0, int l1) {
  BusLens r{BUS_ITEM_OK, KAMD_BUS_FAKE_BARCODE_LEN, 1, 0, 0};
  if (!bus_field_absent(L.umi) && !bus_field_len(L.umi, L.n_umi, l0, l1, &r.umi_len)) { r.status = BUS_ITEM_DROP_UMI; return r; }
  if (!bus_field_absent(L.bc) && !bus_field_len(L.bc, L.n_bc, l0, l1, &r.bc_len)) { r.status = BUS_ITEM_DROP_BC; return r; }
  const int l = L.seq.file ? l1 : l0;
  r.seq_start = L.seq.start;
  if (l > L.seq.start) {
    const int end = (L.seq.stop && L.seq.stop < l) ? L.seq.stop : l;
    r.seq_len = end - L.seq.start;
  }
  return r;
}

// bins of the reference's bc_len[] / umi_len[] histograms: lengths 0 .. 32, longer fields are not counted (:1542, :1615)
KAMD_HD bool bus_len_counted(int len) { return len >= 0 && len <= 32; }

// a present field of an item that is not dropped -> its 2-bit value and flag
KAMD_HD uint64_t bus_field_bits(const kamd_bus_substr* parts, int n, const BusItemView& it, uint32_t* flag) {
  uint64_t r = 0;
  int taken = 0, num_n = 0, pos_n = 0;
  for (int p = 0; p < n && taken < 32; p++) {
    const int f = parts[p].file ? 1 : 0;
    const uint32_t* rec = it.rec[f];
    const int len = parts[p].stop ? parts[p].stop - parts[p].start : it.len[f] - parts[p].start;
    for (int j = 0; j < len && taken < 32; j++, taken++) {
      const int i = parts[p].start + j;
      uint32_t code = (rec[i >> 4] >> (2 * (i & 15))) & 3u;
      if ((rec[it.seq_words + (i >> 5)] >> (i & 31)) & 1u) {
        code = 2;
        if (!num_n) pos_n = taken;
        ++num_n;
      }
      r = (r << 2) | code;
    }
  }
  *flag = num_n ? (uint32_t)(num_n > 3 ? 3 : num_n) | ((uint32_t)(pos_n & 31) << 2) : 0u;
  return r;
}

KAMD_HD kamd_bus_tag bus_item_tag(const kamd_bus_layout& L, const BusItemView& it, const BusLens& ln) {
  kamd_bus_tag t;
  uint32_t f_bc = 0, f_umi = 0;
  t.barcode = bus_field_absent(L.bc) ? 0ULL : bus_field_bits(L.bc, L.n_bc, it, &f_bc);
  if (bus_field_absent(L.umi)) { t.umi = ~0ULL; f_umi = f_bc; }   // (the flag quirk: see the head of this file)
  else t.umi = bus_field_bits(L.umi, L.n_umi, it, &f_umi);
  t.flags = f_bc | (f_umi << 8);
  t.bc_len = (uint16_t)ln.bc_len;
  t.umi_len = (uint16_t)ln.umi_len;
  return t;
}

// word w of the cut's 2-bit half (w < its sequence words - 1: the last one is the flag word); src = the source record, src_seq_words incl. its flag word
KAMD_HD uint32_t bus_cut_seq_word(const uint32_t* src, int src_seq_words, int start, int len, int w) {
  const int b0 = 16 * w;
  if (b0 >= len) return 0u;
  const int g = start + b0, wi = g >> 4, sh = 2 * (g & 15);
  uint32_t v = wi < src_seq_words - 1 ? src[wi] >> sh : 0u;
  if (sh && wi + 1 < src_seq_words - 1) v |= src[wi + 1] << (32 - sh);
  const int rem = len - b0;
  if (rem < 16) v &= (1u << (2 * rem)) - 1u;
  return v;
}
// word w of the cut's mask half; src_mask = the source record's mask words, src_mask_words of them
KAMD_HD uint32_t bus_cut_mask_word(const uint32_t* src_mask, int src_mask_words, int start, int len, int w) {
  const int b0 = 32 * w;
  if (b0 >= len) return 0u;
  const int g = start + b0, wi = g >> 5, sh = g & 31;
  uint32_t v = wi < src_mask_words ? src_mask[wi] >> sh : 0u;
  if (sh && wi + 1 < src_mask_words) v |= src_mask[wi + 1] << (32 - sh);
  const int rem = len - b0;
  if (rem < 32) v &= (1u << rem) - 1u;
  return v;
}

// host only (kamd_bus.cpp): is a layout one that kamd_bus_split takes?  0, or -1 with the reason in err
int bus_layout_check(const kamd_bus_layout* L, char* err, size_t err_cap);

}  // namespace kamd
