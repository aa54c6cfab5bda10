// tests/emu_inflate/inflate_emu.cpp -- TEST INFRASTRUCTURE: drives the device-side inflate's shared logic (kallisto_amd/csrc/kamd_inflate.h:
// decoder, CRC-32, line count and locate) on host buffers, the way the kernels of kamd_inflate.hip do per wavefront.  Never linked into
// libkallisto_amd.so.
#include "../../kallisto_amd/csrc/kamd_inflate.h"

#include <algorithm>
#include <vector>

using namespace kamd::inf;

extern "C" {
// one member: src[0, n) -> out[0, isize); returns the reason (0 = the text is complete and has the trailer's CRC-32)
int inf_emu_member(const uint8_t* src, uint32_t n, uint8_t* out, uint32_t isize, uint32_t crc_expect, uint32_t* crc_out, uint32_t* newlines) {
  if (isize > MAX_ISIZE) return -1;
  std::vector<Work> w(1);
  int r = inflate_member(src, n, out, isize, w[0], 0, 1, [] {});
  if (crc_out) *crc_out = 0;
  if (newlines) *newlines = 0;
  if (r) return r;
  crc_table_fill(w[0].crc_tab, 0, 1);
  uint32_t nl = 0;
  const uint32_t crc = ~crc_slice_term(out, isize, w[0].crc_tab, 0, 1, &nl);
  if (crc_out) *crc_out = crc;
  if (newlines) *newlines = nl;
  return crc == crc_expect ? INF_OK : INF_CRC;
}
// the CRC-32 as `nlanes` lanes compute it: a slice each, the terms combined
uint32_t inf_emu_crc_lanes(const uint8_t* buf, uint32_t n, int nlanes, uint32_t* newlines) {
  uint32_t tab[256], x = 0, nl = 0;
  for (int l = 0; l < nlanes; l++) crc_table_fill(tab, l, nlanes);
  for (int l = 0; l < nlanes; l++) { uint32_t c = 0; x ^= crc_slice_term(buf, n, tab, l, nlanes, &c); nl += c; }
  if (newlines) *newlines = nl;
  return ~x;
}
uint64_t inf_emu_lines(const uint8_t* t, uint64_t lo, uint64_t hi) { return lines_range(t, lo, hi); }
// the offset just behind newline number k (1-based) of t[0, n), through the chunks' partial counts; n when there are fewer, 0 for k = 0
uint64_t inf_emu_locate(const uint8_t* t, uint64_t n, uint64_t k) {
  if (k == 0) return 0;
  const uint64_t nc = (n + TEXT_CHUNK - 1) / TEXT_CHUNK;
  std::vector<uint32_t> counts(nc);
  for (uint64_t c = 0; c < nc; c++) counts[c] = (uint32_t)lines_range(t, c * TEXT_CHUNK, std::min(n, (c + 1) * TEXT_CHUNK));
  uint64_t r = 0;
  const uint64_t c = locate_chunk(counts.data(), nc, k, &r);
  if (c == nc) return n;
  return locate_in(t, c * TEXT_CHUNK, std::min(n, (c + 1) * TEXT_CHUNK), r);
}
// kamd_text_cut on host texts
void inf_emu_text_cut(const uint8_t* const* t, const uint64_t* n, int n_files, uint64_t max_records, uint64_t* n_records, uint64_t* end) {
  uint64_t lines[2] = {0, 0};
  for (int f = 0; f < n_files; f++) lines[f] = lines_range(t[f], 0, n[f]);
  *n_records = records_of(lines, n_files, max_records);
  for (int f = 0; f < n_files; f++) end[f] = inf_emu_locate(t[f], n[f], 4 * *n_records);
}
}
