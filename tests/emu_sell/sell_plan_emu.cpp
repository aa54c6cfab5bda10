// tests/emu_sell/sell_plan_emu.cpp -- TEST INFRASTRUCTURE: the plan k_em_sell iterates, built on the CPU by the steps the device set-up is made
// of (kamd_em_local.h build_plan_steps_host, then kamd_em_sell.h from_csr_plan), reduced to what a test needs to know about its inputs:
// the shape of every group's tables.
#include "../../kallisto_amd/csrc/kamd_em_local.h"
#include "../../kallisto_amd/csrc/kamd_em_sell.h"

extern "C" {
static const int SELL_STAT_WORDS = 12;
// per group: rows, transcripts, entries, row slices, column slices, row stream u16, column stream u16, padding entries in the row stream,
// ... in the column stream, row slices with lane metadata, the largest segment id in the row streams' lane metadata, column slices with metadata
// returns the number of groups (< 0: the plan could not be built); *n_small: groups of the small size class (one wavefront each)
int emu_sell_plan_stats(const uint64_t* ec_off, const uint32_t* ec_ids, const uint32_t* counts, uint64_t n_ecs, const double* eff, uint64_t T,
                        uint64_t budget_bytes, uint64_t target_nnz, uint32_t small_limit, uint64_t target_small, uint32_t cap, uint32_t* stats,
                        uint32_t max_groups, uint32_t* n_small) {
  namespace L = kamd_em_local;
  namespace S = kamd_em_sell;
  L::Plan C;
  if (L::build_plan_steps_host(ec_off, ec_ids, counts, nullptr, n_ecs, eff, T, budget_bytes, target_nnz, &C, small_limit, target_small)) return -1;
  S::Plan P;
  if (S::from_csr_plan(C, budget_bytes, &P, cap)) return -2;
  if (P.n_groups > max_groups) return -3;
  *n_small = P.n_small;
  for (uint32_t g = 0; g < P.n_groups; g++) {
    uint32_t* o = stats + (size_t)g * SELL_STAT_WORDS;
    o[0] = P.row_base[g + 1] - P.row_base[g]; o[1] = P.tr_base[g + 1] - P.tr_base[g]; o[2] = (uint32_t)(C.nz_base[g + 1] - C.nz_base[g]);
    o[3] = P.rslice_base[g + 1] - P.rslice_base[g]; o[4] = P.cslice_base[g + 1] - P.cslice_base[g];
    o[5] = (uint32_t)(P.rell_base[g + 1] - P.rell_base[g]); o[6] = (uint32_t)(P.cell_base[g + 1] - P.cell_base[g]);
    for (int dir = 0; dir < 2; dir++) {
      const uint32_t* desc = (dir ? P.cdesc.data() + 2 * (size_t)P.cslice_base[g] : P.rdesc.data() + 2 * (size_t)P.rslice_base[g]);
      const uint16_t* ell = dir ? P.cell.data() + P.cell_base[g] : P.rell.data() + P.rell_base[g];
      uint32_t pads = 0, metas = 0, max_seg = 0;
      for (uint32_t s = 0; s < o[3 + dir]; s++) {
        const uint32_t d0 = desc[2 * s], width = desc[2 * s + 1] & 0xFFFFu, off = d0 & ~S::DESC_META;
        const bool meta = (d0 & S::DESC_META) != 0;
        if (meta) {
          ++metas;
          for (uint32_t l = 0; l < S::SELL_LANES; l++) {
            const uint32_t w = (uint32_t)ell[off + 2 * l] | ((uint32_t)ell[off + 2 * l + 1] << 16);
            if ((w & S::META_ACTIVE) && (w & 0xFFFFu) > max_seg) max_seg = w & 0xFFFFu;
          }
        }
        const uint16_t* e = ell + off + (meta ? 2 * S::SELL_META_WORDS : 0u);
        for (uint32_t i = 0; i < S::quad_width(width) * S::SELL_LANES; i++) pads += e[i] == S::SELL_PAD;
      }
      if (dir == 0) { o[7] = pads; o[9] = metas; o[10] = max_seg; } else { o[8] = pads; o[11] = metas; }
    }
  }
  return (int)P.n_groups;
}
}
