// kamd_busgenes.hip -- BUS records to a cells x genes matrix on the device (kamd_bus_genes_create, kamd_bus_count_genes): what `bustools count
// --genecounts -g t2g.txt` does with the sorted records of kamd_bus_sort.  The gene lists and the rule of a group are those of kamd_busgenes.h,
// rows and groups those of kamd_bussort.h; this file is the kernels around them.  Neither call reads or writes the EC state, the counts, the tuple
// table or the fragment-length sample.
//
// kamd_bus_genes_create (a plan step, once per run): the map and the classes' CSR are checked on the host and uploaded, then
//   k_gl_count / k_bus_scan / k_gl_scatter   one thread per entry of the CSR: an entry whose transcript has a gene becomes the key
//                     {barcode = class, umi = gene} (the class of entry i by a binary search of the offsets), compact and in input order
//   kamd_bus_sort's passes and collapse over the keys: the distinct (class, gene) pairs, by class and then by gene
//   k_gl_offsets      one thread per class: its list begins at the first pair of a class >= its own (binary search: classes without a gene
//                     need no walk); one thread per pair: its gene -> ids; classes without a gene are counted, the longest list kept (atomicMax)
//   Three synchronisations: the number of keys, then the sort's two.
// kamd_bus_count_genes (its input in key order):
//   k_cnt_heads / k_bus_scan x 2 / k_cnt_starts   as kamd_bus_count: rows (into scratch: nothing of the caller's is written before the call is
//                     known to succeed) and group starts
//   k_gen_thread      one thread per group (READS: per record).  A group of at most GENES_THREAD_MAX_RECORDS records: its classes are
//                     range-checked, a group of one record is settled by the length of its list and the list's first id, a group whose smallest
//                     list has at most GENES_THREAD_MAX_LIST genes by gene_of_group.  Every other group goes to the list: ranks by ballot
//                     within the block, the block's place by one atomicAdd (the list's order varies from run to run; nothing is derived from
//                     it, results are written by group index)
//   k_gen_wave        one wavefront per listed group, on a fixed grid (the length of the list stays on the device).  The lanes range-check the
//                     group's classes and find the record with the smallest list (min-reduce of (length, record): the first wins a tie).  Then
//                     either the lanes take that list's candidates 64 at a time and each looks its candidate up in every other record's list,
//                     leaving at the first list that lacks it, the survivors counted by ballot and __popcll; or, where the group has so many
//                     records that this is less work, the candidates are taken one by one and the lanes share the records, 64 at a time, until
//                     one lacks the candidate.  Either way the wavefront stops at the second survivor, and no loop is longer than the group's
//                     records or its smallest list.
//   k_gen_count / k_bus_scan / k_gen_emit   the heads of the groups with a gene (READS: the records) -> unit records {row, 0, gene, 1 or count,
//                     0, row}, compact and in input order; the three outcomes are counted (integer adds, no value returned)
//   then kamd_bus_sort's passes and collapse over the unit records and k_cnt_entries, as kamd_bus_count; the rows are copied out last.
//   The host reads the counters behind k_gen_emit (an unsorted input or a class outside the table ends the call there), the sort synchronises
//   twice more.
// All launches are separate launches on the context stream; nothing waits for another workgroup inside a launch.
#include "kamd_bussort_dev.h"
#include "kamd_busgenes.h"

struct kamd_bus_genes {
  u64* off = nullptr;
  int32_t* ids = nullptr;
  u64 n_classes = 0, n_pairs = 0;
  kamd_bus_genes_stats stats{};
};

namespace {

constexpr int WAVES = BLOCK / 64;

struct GeneCounters {
  u64 n_keys, n_empty;                                               // kamd_bus_genes_create
  u64 n_bad, n_list, n_units, n_counted, n_no_gene, n_multi_gene;    // kamd_bus_count_genes
  u32 max_list, pad;
};

// ---- kamd_bus_genes_create ----
__global__ __launch_bounds__(BLOCK) void k_gl_count(const int32_t* __restrict__ tr_gene, const u32* __restrict__ ec_ids, u64 n_entries, u32* __restrict__ blk_cnt) {
  const u64 i = (u64)blockIdx.x * BLOCK + threadIdx.x;
  const bool valid = i < n_entries && tr_gene[ec_ids[i]] >= 0;   // (every id is below n_targets: checked on the host)
  const int cnt = __syncthreads_count(valid);
  if (threadIdx.x == 0) blk_cnt[blockIdx.x] = (u32)cnt;
}

__global__ __launch_bounds__(BLOCK) void k_gl_scatter(const int32_t* __restrict__ tr_gene, const u64* __restrict__ ec_off, const u32* __restrict__ ec_ids, u64 n_entries,
                                                      u64 n_classes, const u32* __restrict__ blk_off, kamd_bus_record* __restrict__ keys) {
  __shared__ u32 s_w[BUS_WAVES];
  const u64 i = (u64)blockIdx.x * BLOCK + threadIdx.x;
  const int32_t gene = i < n_entries ? tr_gene[ec_ids[i]] : -1;
  const u32 rank = block_rank(gene >= 0, s_w);
  if (gene < 0) return;
  const u64 cls = kamd::csr_row_of((const uint64_t*)ec_off, (uint64_t)n_classes, (uint64_t)i);   // (i < off[n_classes]: cls < n_classes)
  store_rec(keys + ((u64)blk_off[blockIdx.x] + rank), q_of(kamd::gene_pair_record(cls, gene)));      // (the keys before this one: at most i)
}

// the first pair of a class >= cls
__device__ __forceinline__ u64 pair_lower_bound(const kamd_bus_record* pairs, u64 n_pairs, u64 cls) {
  u64 lo = 0, hi = n_pairs;
  while (lo < hi) { const u64 mid = (lo + hi) >> 1; if (pairs[mid].barcode < cls) lo = mid + 1; else hi = mid; }
  return lo;
}

__global__ __launch_bounds__(BLOCK) void k_gl_offsets(const kamd_bus_record* __restrict__ pairs, u64 n_pairs, u64 n_classes, u64* __restrict__ off, int32_t* __restrict__ ids,
                                                      GeneCounters* ctr) {
  const u64 t = (u64)blockIdx.x * BLOCK + threadIdx.x;
  if (t < n_pairs) ids[t] = (int32_t)(u32)pairs[t].umi;
  bool empty = false;
  u32 len = 0;
  if (t <= n_classes) {
    const u64 lo = pair_lower_bound(pairs, n_pairs, t);
    off[t] = lo;   // (t <= n_classes: inside [n_classes + 1])
    if (t < n_classes) { len = (u32)(pair_lower_bound(pairs, n_pairs, t + 1) - lo); empty = len == 0; }
  }
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) len = max(len, (u32)__shfl_xor((int)len, d, 64));
  if (lane_id() == 0 && len) atomicMax(&ctr->max_list, len);
  const int n_empty = __syncthreads_count(empty);
  if (threadIdx.x == 0 && n_empty) atomicAdd(&ctr->n_empty, (u64)n_empty);
}

// ---- kamd_bus_count_genes ----
__global__ __launch_bounds__(BLOCK) void k_gen_thread(kamd::GeneLists t, const kamd_bus_record* __restrict__ rec, u64 n, int mode, const SortCounters* __restrict__ sctr,
                                                      const u32* __restrict__ gstart, GeneCounters* gctr, int32_t* __restrict__ gene_of, u32* __restrict__ list) {
  __shared__ u32 s_w[BUS_WAVES];
  __shared__ u32 s_base;
  if (sctr->n_unsorted) return;   // (uniform)
  const u64 g = (u64)blockIdx.x * BLOCK + threadIdx.x;
  const u64 n_grp = mode == KAMD_BUS_COUNT_READS ? n : min(sctr->n_groups, n);
  bool bad = false, listed = false;
  if (g < n_grp) {
    const u64 first = mode == KAMD_BUS_COUNT_READS ? g : (u64)gstart[g];
    const u64 m = mode == KAMD_BUS_COUNT_READS ? 1 : (u64)gstart[g + 1] - first;   // (first + m <= n: k_cnt_starts)
    int32_t gene = kamd::GENE_NONE;
    if (m <= kamd::GENES_THREAD_MAX_RECORDS) {
      auto class_at = [&](u64 k) { return rec[first + k].ec; };
      for (u64 k = 0; k < m; k++) bad = bad || !kamd::gene_class_ok(t, class_at(k));
      if (!bad) {
        if (m == 1) gene = kamd::gene_of_class(t, class_at(0));
        else {
          uint32_t min_len = 0;
          kamd::gene_group_pivot(t, (uint64_t)m, class_at, &min_len);
          if (kamd::gene_group_small((uint64_t)m, min_len)) gene = kamd::gene_of_group(t, (uint64_t)m, class_at);
          else listed = true;
        }
      }
    } else listed = true;
    if (!listed) gene_of[g] = gene;   // (g < n: inside [n])
  }
  const u32 rank = block_rank(listed, s_w);
  if (threadIdx.x == 0) {
    u32 cnt = 0;
    for (int w = 0; w < BUS_WAVES; w++) cnt += s_w[w];
    s_base = cnt ? (u32)atomicAdd(&gctr->n_list, (u64)cnt) : 0u;
  }
  const int n_bad = __syncthreads_count(bad);   // (a barrier: s_base is written)
  if (listed) {
    const u64 at = (u64)s_base + rank;
    if (at < n) list[at] = (u32)g;   // (the blocks' counts sum to at most n: inside the list of n entries)
  }
  if (threadIdx.x == 0 && n_bad) atomicAdd(&gctr->n_bad, (u64)n_bad);
}

__device__ __forceinline__ u64 shfl_xor_u64(u64 v, int d) { return ((u64)(u32)__shfl_xor((int)(v >> 32), d, 64) << 32) | (u32)__shfl_xor((int)v, d, 64); }

__global__ __launch_bounds__(BLOCK) void k_gen_wave(kamd::GeneLists t, const kamd_bus_record* __restrict__ rec, u64 n, const SortCounters* __restrict__ sctr,
                                                    const u32* __restrict__ gstart, GeneCounters* gctr, const u32* __restrict__ list, int32_t* __restrict__ gene_of) {
  if (sctr->n_unsorted) return;   // (uniform)
  const int lane = lane_id();
  const u64 n_list = min(gctr->n_list, n), n_grp = min(sctr->n_groups, n), stride = (u64)gridDim.x * WAVES;
  for (u64 li = (u64)blockIdx.x * WAVES + (threadIdx.x >> 6); li < n_list; li += stride) {   // (uniform over the wavefront, and so is all control flow below)
    const u64 g = list[li];
    if (g >= n_grp) continue;
    const u64 first = gstart[g], end = gstart[g + 1];
    if (first >= end || end > n) continue;
    const u64 m = end - first;
    // the classes in range, and the record with the smallest list: a lane sees its records in ascending order, the reduction prefers the lower record
    bool bad = false;
    u64 key = ~0ULL;   // (length << 32) | record
    for (u64 k = lane; k < m; k += 64) {
      const int32_t c = rec[first + k].ec;
      if (!kamd::gene_class_ok(t, c)) bad = true;
      else key = min(key, ((u64)kamd::gene_list_len(t, c) << 32) | k);
    }
    if (__ballot(bad)) {
      if (lane == 0) { atomicAdd(&gctr->n_bad, 1ULL); gene_of[g] = kamd::GENE_NONE; }
      continue;
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) key = min(key, shfl_xor_u64(key, d));
    const u32 min_len = (u32)(key >> 32);
    const u64 pivot = key & 0xFFFFFFFFULL;   // (< m: every record was in range)
    const int32_t* cand = t.ids + t.off[rec[first + pivot].ec];
    u32 survivors = 0;
    int32_t gene = kamd::GENE_NONE;
    const bool by_records = (u64)min_len * ((m + 63) / 64) < (u64)((min_len + 63u) / 64u) * m;
    if (!by_records) {
      for (u32 j0 = 0; j0 < min_len && survivors < 2; j0 += 64) {
        const u32 j = j0 + (u32)lane;
        bool alive = j < min_len;
        const int32_t x = alive ? cand[j] : 0;
        for (u64 k = 0; k < m; k++) {
          if (!__ballot(alive)) break;
          if (k == pivot) continue;
          const int32_t c = rec[first + k].ec;
          if (alive) alive = kamd::gene_list_has(t, c, x);
        }
        const u64 b = __ballot(alive);
        if (b) {
          const int32_t gx = __shfl(x, __ffsll((unsigned long long)b) - 1, 64);
          if (survivors == 0) gene = gx;
          survivors += (u32)__popcll(b);
        }
      }
    } else {
      for (u32 j = 0; j < min_len && survivors < 2; j++) {
        const int32_t x = cand[j];
        bool miss = false;
        for (u64 k0 = 0; k0 < m; k0 += 64) {
          const u64 k = k0 + (u64)lane;
          if (k < m && k != pivot) miss = !kamd::gene_list_has(t, rec[first + k].ec, x);
          if (__ballot(miss)) break;
        }
        if (!__ballot(miss)) { if (survivors == 0) gene = x; ++survivors; }
      }
    }
    if (lane == 0) gene_of[g] = survivors == 1 ? gene : (survivors == 0 ? kamd::GENE_NONE : kamd::GENE_MULTI);   // (g < n_grp <= n)
  }
}

// the gene that record i stands for, where it stands for a group: UMIS the head of a group, READS every record; `before`: the group heads of the
// block before this thread
struct GroupGene { bool is_group; int32_t gene; };
__device__ __forceinline__ GroupGene group_gene(u64 i, u64 n, int mode, bool head, u32 before, const u32* blk_grp, const int32_t* gene_of) {
  GroupGene r{false, kamd::GENE_NONE};
  if (i >= n) return r;
  if (mode == KAMD_BUS_COUNT_READS) { r.is_group = true; r.gene = gene_of[i]; }
  else if (head) { r.is_group = true; r.gene = gene_of[(u64)blk_grp[blockIdx.x] + before]; }   // (the heads before this one: its group, < n_groups)
  return r;
}

__global__ __launch_bounds__(BLOCK) void k_gen_count(const kamd_bus_record* __restrict__ rec, u64 n, int mode, const u32* __restrict__ blk_grp, const SortCounters* __restrict__ sctr,
                                                     const int32_t* __restrict__ gene_of, GeneCounters* gctr, u32* __restrict__ blk_unit) {
  __shared__ u32 s_w[BUS_WAVES];
  if (sctr->n_unsorted) return;   // (uniform)
  const u64 i = (u64)blockIdx.x * BLOCK + threadIdx.x;
  kamd_bus_record me;
  const Heads h = rec_heads(rec, i, n, &me);
  const u32 before = block_rank(h.grp, s_w);
  const GroupGene gg = group_gene(i, n, mode, h.grp, before, blk_grp, gene_of);
  const int n_unit = __syncthreads_count(gg.is_group && gg.gene >= 0), n_none = __syncthreads_count(gg.is_group && gg.gene == kamd::GENE_NONE),
            n_multi = __syncthreads_count(gg.is_group && gg.gene == kamd::GENE_MULTI);
  if (threadIdx.x == 0) {
    blk_unit[blockIdx.x] = (u32)n_unit;
    if (n_unit) atomicAdd(&gctr->n_counted, (u64)n_unit);
    if (n_none) atomicAdd(&gctr->n_no_gene, (u64)n_none);
    if (n_multi) atomicAdd(&gctr->n_multi_gene, (u64)n_multi);
  }
}

__global__ __launch_bounds__(BLOCK) void k_gen_emit(const kamd_bus_record* __restrict__ rec, u64 n, int mode, const u32* __restrict__ blk_bc, const u32* __restrict__ blk_grp,
                                                    const u32* __restrict__ blk_unit, const SortCounters* __restrict__ sctr, const int32_t* __restrict__ gene_of,
                                                    kamd_bus_record* __restrict__ units) {
  __shared__ u32 s_w[3][BUS_WAVES];
  if (sctr->n_unsorted) return;   // (uniform)
  const u64 i = (u64)blockIdx.x * BLOCK + threadIdx.x;
  kamd_bus_record me;
  const Heads h = rec_heads(rec, i, n, &me);
  const u32 r_bc = block_rank(h.bc, s_w[0]), r_grp = block_rank(h.grp, s_w[1]);
  const GroupGene gg = group_gene(i, n, mode, h.grp, r_grp, blk_grp, gene_of);
  const bool unit = gg.is_group && gg.gene >= 0;
  const u32 r_unit = block_rank(unit, s_w[2]);
  if (!unit) return;
  const u32 row = blk_bc[blockIdx.x] + r_bc + (h.bc ? 1u : 0u) - 1u;
  me.ec = gg.gene;
  store_rec(units + ((u64)blk_unit[blockIdx.x] + r_unit), q_of(kamd::bus_unit_record(me, row, mode)));   // (compact: inside [n])
}

bool misaligned(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) != 0; }
bool owns(const kamd_ctx* c, const kamd_bus_genes* g) { return std::find(c->gene_tables.begin(), c->gene_tables.end(), g) != c->gene_tables.end(); }
void table_free(kamd_bus_genes* g) {
  if (g->off) (void)hipFree(g->off);
  if (g->ids) (void)hipFree(g->ids);
  delete g;
}

// device allocations of a call, freed when it ends
struct Temps {
  std::vector<void*> v;
  ~Temps() { for (void* p : v) (void)hipFree(p); }
  template <class T> int alloc(T** out, u64 n) {
    void* p = nullptr;
    HIPC(hipMalloc(&p, std::max<u64>(n, 1) * sizeof(T)));
    v.push_back(p);
    *out = reinterpret_cast<T*>(p);
    return 0;
  }
};

}  // namespace

namespace kamdi {
void gene_tables_free_all(kamd_ctx* c) {
  for (kamd_bus_genes* g : c->gene_tables) table_free(g);
  c->gene_tables.clear();
}
}  // namespace kamdi

extern "C" int kamd_bus_genes_create(kamd_ctx* c, const int32_t* h_tr_gene, uint64_t n_targets, int32_t n_genes, const uint64_t* h_ec_off, const uint32_t* h_ec_ids,
                                     uint64_t n_classes, kamd_bus_genes** out, kamd_bus_genes_stats* stats) {
  if (out) *out = nullptr;
  if (stats) memset(stats, 0, sizeof *stats);
  if (!c || !out || !h_ec_off || (n_targets && !h_tr_gene)) return kamd::fail(-1, "kamd_bus_genes_create: null argument");
  if (n_genes < 0) return kamd::fail(-1, "kamd_bus_genes_create: a negative number of genes");
  if (n_classes >= 0x7FFFFFFFULL) return kamd::fail(-1, "kamd_bus_genes_create: a table holds fewer than 2^31 - 1 classes");
  for (u64 t = 0; t < n_targets; t++)
    if (h_tr_gene[t] < -1 || h_tr_gene[t] >= n_genes)
      return kamd::fail(-1, "kamd_bus_genes_create: transcript " + std::to_string(t) + " has gene " + std::to_string(h_tr_gene[t]) + ", neither -1 nor in [0, " +
                                std::to_string(n_genes) + ")");
  if (h_ec_off[0] != 0) return kamd::fail(-1, "kamd_bus_genes_create: the offsets must begin at 0");
  for (u64 e = 0; e < n_classes; e++)
    if (h_ec_off[e + 1] < h_ec_off[e]) return kamd::fail(-1, "kamd_bus_genes_create: the offsets decrease at class " + std::to_string(e));
  const u64 n_entries = h_ec_off[n_classes];
  if (n_entries >= 0xFFFFFFFFULL) return kamd::fail(-1, "kamd_bus_genes_create: the classes hold fewer than 2^32 - 1 entries");
  if (n_entries && !h_ec_ids) return kamd::fail(-1, "kamd_bus_genes_create: null argument");
  for (u64 i = 0; i < n_entries; i++)
    if (h_ec_ids[i] >= n_targets)
      return kamd::fail(-1, "kamd_bus_genes_create: entry " + std::to_string(i) + " names transcript " + std::to_string(h_ec_ids[i]) + " of " + std::to_string(n_targets));
  if (int rc = bus_events_begin(c)) return rc;
  const unsigned nb = grid_for(n_entries, BLOCK);
  if (int rc = c->bgen_ctr.ensure(sizeof(GeneCounters), 0, c->stream)) return rc;
  if (int rc = c->bgen_blk.ensure((size_t)std::max(nb, 1u) * sizeof(u32), 0, c->stream)) return rc;
  GeneCounters* ctr = c->bgen_ctr.as<GeneCounters>();
  u32* blk = c->bgen_blk.as<u32>();
  Temps tmp;
  int32_t* d_tr = nullptr; u64* d_off = nullptr; u32* d_ids = nullptr; kamd_bus_record* keys = nullptr;
  if (int rc = tmp.alloc(&d_tr, n_targets)) return rc;
  if (int rc = tmp.alloc(&d_off, n_classes + 1)) return rc;
  if (int rc = tmp.alloc(&d_ids, n_entries)) return rc;
  if (int rc = tmp.alloc(&keys, n_entries)) return rc;
  kamd_bus_genes* g = new kamd_bus_genes;
  g->n_classes = n_classes;
  GeneCounters h{};
  u64 n_pairs = 0;
  auto run = [&]() -> int {
    HIPC(hipMalloc((void**)&g->off, (n_classes + 1) * sizeof(u64)));
    HIPC(hipMemsetAsync(ctr, 0, sizeof *ctr, c->stream));
    if (n_targets) HIPC(hipMemcpyAsync(d_tr, h_tr_gene, n_targets * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    HIPC(hipMemcpyAsync(d_off, h_ec_off, (n_classes + 1) * sizeof(u64), hipMemcpyHostToDevice, c->stream));
    if (n_entries) {
      HIPC(hipMemcpyAsync(d_ids, h_ec_ids, n_entries * sizeof(u32), hipMemcpyHostToDevice, c->stream));
      hipLaunchKernelGGL(k_gl_count, dim3(nb), dim3(BLOCK), 0, c->stream, (const int32_t*)d_tr, (const u32*)d_ids, (u64)n_entries, blk);
      hipLaunchKernelGGL(k_bus_scan, dim3(1), dim3(BLOCK), 0, c->stream, blk, (u64)nb, &ctr->n_keys);
      hipLaunchKernelGGL(k_gl_scatter, dim3(nb), dim3(BLOCK), 0, c->stream, (const int32_t*)d_tr, (const u64*)d_off, (const u32*)d_ids, (u64)n_entries, (u64)n_classes,
                         (const u32*)blk, keys);
      HIPC(hipGetLastError());
      HIPC(hipMemcpyAsync(&h, ctr, sizeof h, hipMemcpyDeviceToHost, c->stream));
      HIPC(hipStreamSynchronize(c->stream));   // the number of keys
      if (h.n_keys > n_entries) return kamd::fail(-4, "kamd_bus_genes_create: more keys than entries");
      if (h.n_keys)
        if (int rc = bus_sort_records(c, keys, h.n_keys, nullptr, 0, 1, &n_pairs, nullptr, "kamd_bus_genes_create")) return rc;
    }
    HIPC(hipMalloc((void**)&g->ids, std::max<u64>(n_pairs, 1) * sizeof(int32_t)));
    const u64 n_thr = std::max<u64>(n_classes + 1, n_pairs);
    hipLaunchKernelGGL(k_gl_offsets, dim3(grid_for(n_thr, BLOCK)), dim3(BLOCK), 0, c->stream, (const kamd_bus_record*)keys, (u64)n_pairs, (u64)n_classes, g->off, g->ids, ctr);
    HIPC(hipGetLastError());
    HIPC(hipMemcpyAsync(&h, ctr, sizeof h, hipMemcpyDeviceToHost, c->stream));
    return 0;
  };
  float ms = 0.f;
  int rc = run();
  if (!rc) rc = bus_events_end(c, &ms);   // (synchronises: the counters are here, the temporaries may go)
  else (void)hipStreamSynchronize(c->stream);
  if (rc) { table_free(g); return rc; }
  g->n_pairs = n_pairs;
  g->stats.n_classes = n_classes; g->stats.n_entries_in = n_entries; g->stats.n_pairs = n_pairs; g->stats.n_empty = h.n_empty; g->stats.max_list = h.max_list;
  g->stats.n_genes = n_genes; g->stats.last_ms = ms;
  c->gene_tables.push_back(g);
  if (stats) *stats = g->stats;
  *out = g;
  return 0;
}

extern "C" int kamd_bus_genes_free(kamd_ctx* c, kamd_bus_genes* g) {
  if (!c) return kamd::fail(-1, "kamd_bus_genes_free: null context");
  if (!g) return 0;
  if (!owns(c, g)) return kamd::fail(-1, "kamd_bus_genes_free: not a gene table of this context");
  HIPC(hipSetDevice(c->device));
  HIPC(hipStreamSynchronize(c->stream));   // (a kamd_bus_count_genes of the caller's may still read it)
  c->gene_tables.erase(std::find(c->gene_tables.begin(), c->gene_tables.end(), g));
  table_free(g);
  return 0;
}

extern "C" int kamd_bus_genes_download(kamd_ctx* c, const kamd_bus_genes* g, uint64_t* h_off, int32_t* h_ids) {
  if (!c || !g || !h_off) return kamd::fail(-1, "kamd_bus_genes_download: null argument");
  if (!owns(c, g)) return kamd::fail(-1, "kamd_bus_genes_download: not a gene table of this context");
  if (g->n_pairs && !h_ids) return kamd::fail(-1, "kamd_bus_genes_download: null argument");
  HIPC(hipSetDevice(c->device));
  HIPC(hipMemcpyAsync(h_off, g->off, (g->n_classes + 1) * sizeof(u64), hipMemcpyDeviceToHost, c->stream));
  if (g->n_pairs) HIPC(hipMemcpyAsync(h_ids, g->ids, g->n_pairs * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
  HIPC(hipStreamSynchronize(c->stream));
  return 0;
}

extern "C" int kamd_bus_count_genes(kamd_ctx* c, const kamd_bus_genes* tab, const kamd_bus_record* d_sorted, uint64_t n, int mode, uint64_t* d_barcodes,
                                    kamd_bus_entry* d_entries, kamd_bus_gene_count_stats* out) {
  if (out) memset(out, 0, sizeof *out);
  if (!c || !tab) return kamd::fail(-1, "kamd_bus_count_genes: null argument");
  if (!owns(c, tab)) return kamd::fail(-1, "kamd_bus_count_genes: not a gene table of this context");
  if (mode != KAMD_BUS_COUNT_UMIS && mode != KAMD_BUS_COUNT_READS) return kamd::fail(-1, "kamd_bus_count_genes: mode must be KAMD_BUS_COUNT_UMIS or KAMD_BUS_COUNT_READS");
  if (n >= 0xFFFFFFFFULL) return kamd::fail(-1, "kamd_bus_count_genes: a call takes fewer than 2^32 - 1 records");
  if (n == 0) return 0;
  if (!d_sorted || !d_barcodes || !d_entries) return kamd::fail(-1, "kamd_bus_count_genes: null argument");
  if (misaligned(d_sorted)) return kamd::fail(-1, "kamd_bus_count_genes: the records must be 16-byte aligned");
  if (int rc = bus_events_begin(c)) return rc;
  for (hipEvent_t& e : c->bgen_ev) if (!e) HIPC(hipEventCreate(&e));
  const u64 nb = grid_for(n, BLOCK);
  if (int rc = c->bgen_blk.ensure(3 * nb * sizeof(u32), 0, c->stream)) return rc;
  if (int rc = c->bgen_ctr.ensure(sizeof(GeneCounters), 0, c->stream)) return rc;
  if (int rc = c->bgen_gene.ensure(n * sizeof(int32_t), 0, c->stream)) return rc;
  if (int rc = c->bgen_list.ensure(n * sizeof(u32), 0, c->stream)) return rc;
  if (int rc = c->bgen_rows.ensure(n * sizeof(u64), 0, c->stream)) return rc;
  if (int rc = c->bcnt_units.ensure(n * sizeof(kamd_bus_record), 0, c->stream)) return rc;
  if (int rc = c->bcnt_gstart.ensure((n + 1) * sizeof(u32), 0, c->stream)) return rc;
  if (int rc = c->bsort_ctr.ensure(sizeof(SortCounters), 0, c->stream)) return rc;
  SortCounters* sctr = c->bsort_ctr.as<SortCounters>();
  GeneCounters* gctr = c->bgen_ctr.as<GeneCounters>();
  HIPC(hipMemsetAsync(sctr, 0, sizeof *sctr, c->stream));
  HIPC(hipMemsetAsync(gctr, 0, sizeof *gctr, c->stream));
  u32 *blk_bc = c->bgen_blk.as<u32>(), *blk_grp = blk_bc + nb, *blk_unit = blk_grp + nb;
  kamd_bus_record* units = c->bcnt_units.as<kamd_bus_record>();
  u32 *gstart = c->bcnt_gstart.as<u32>(), *list = c->bgen_list.as<u32>();
  int32_t* gene_of = c->bgen_gene.as<int32_t>();
  u64* rows = c->bgen_rows.as<u64>();
  const kamd::GeneLists t{(const uint64_t*)tab->off, tab->ids, (uint64_t)tab->n_classes};
  // k_gen_wave: a wavefront per listed group, at most sixteen workgroups per compute unit and no more wavefronts than half the records (a listed group has two)
  const unsigned wave_grid = (unsigned)std::min<u64>(grid_for((n + 1) / 2, WAVES), (u64)std::max(c->n_cus, 1) * 16);
  const dim3 g((unsigned)nb), th(BLOCK);
  hipLaunchKernelGGL(k_cnt_heads, g, th, 0, c->stream, d_sorted, (u64)n, blk_bc, blk_grp, sctr);
  hipLaunchKernelGGL(k_bus_scan, dim3(1), th, 0, c->stream, blk_bc, nb, &sctr->n_barcodes);
  hipLaunchKernelGGL(k_bus_scan, dim3(1), th, 0, c->stream, blk_grp, nb, &sctr->n_groups);
  hipLaunchKernelGGL(k_cnt_starts, g, th, 0, c->stream, d_sorted, (u64)n, (const u32*)blk_bc, (const u32*)blk_grp, (const SortCounters*)sctr, rows, gstart);
  HIPC(hipEventRecord(c->bgen_ev[0], c->stream));
  hipLaunchKernelGGL(k_gen_thread, g, th, 0, c->stream, t, d_sorted, (u64)n, mode, (const SortCounters*)sctr, (const u32*)gstart, gctr, gene_of, list);
  if (mode == KAMD_BUS_COUNT_UMIS)
    hipLaunchKernelGGL(k_gen_wave, dim3(wave_grid), th, 0, c->stream, t, d_sorted, (u64)n, (const SortCounters*)sctr, (const u32*)gstart, gctr, (const u32*)list, gene_of);
  HIPC(hipEventRecord(c->bgen_ev[1], c->stream));
  hipLaunchKernelGGL(k_gen_count, g, th, 0, c->stream, d_sorted, (u64)n, mode, (const u32*)blk_grp, (const SortCounters*)sctr, (const int32_t*)gene_of, gctr, blk_unit);
  hipLaunchKernelGGL(k_bus_scan, dim3(1), th, 0, c->stream, blk_unit, nb, &gctr->n_units);
  hipLaunchKernelGGL(k_gen_emit, g, th, 0, c->stream, d_sorted, (u64)n, mode, (const u32*)blk_bc, (const u32*)blk_grp, (const u32*)blk_unit, (const SortCounters*)sctr,
                     (const int32_t*)gene_of, units);
  SortCounters hs{};
  GeneCounters hg{};
  HIPC(hipMemcpyAsync(&hg, gctr, sizeof hg, hipMemcpyDeviceToHost, c->stream));
  if (int rc = bus_read_counters(c, &hs)) return rc;   // the one synchronisation for the counters (the sort below starts its own)
  if (hs.n_unsorted)
    return kamd::fail(-4, "kamd_bus_count_genes: " + std::to_string(hs.n_unsorted) + " records lie before their predecessor in key order: the input is not sorted; nothing counted");
  if (hg.n_bad)
    return kamd::fail(-4, "kamd_bus_count_genes: " + std::to_string(hg.n_bad) + " groups hold a record whose class is outside the table's [0, " +
                              std::to_string(tab->n_classes) + "); nothing counted");
  u64 n_entries = 0;
  if (hg.n_units) {
    if (int rc = bus_sort_records(c, units, hg.n_units, nullptr, 0, 1, &n_entries, nullptr, "kamd_bus_count_genes")) return rc;
    hipLaunchKernelGGL(k_cnt_entries, dim3(grid_for(n_entries, BLOCK)), th, 0, c->stream, (const kamd_bus_record*)units, n_entries, d_entries);
    HIPC(hipGetLastError());
  }
  HIPC(hipMemcpyAsync(d_barcodes, rows, hs.n_barcodes * sizeof(u64), hipMemcpyDeviceToDevice, c->stream));
  float ms = 0.f, resolve_ms = 0.f;
  if (int rc = bus_events_end(c, &ms)) return rc;
  HIPC(hipEventElapsedTime(&resolve_ms, c->bgen_ev[0], c->bgen_ev[1]));
  if (out) {
    out->n_records = n; out->n_barcodes = hs.n_barcodes; out->n_entries = n_entries; out->n_umis = mode == KAMD_BUS_COUNT_READS ? n : hs.n_groups;
    out->n_counted = hg.n_counted; out->n_no_gene = hg.n_no_gene; out->n_multi_gene = hg.n_multi_gene; out->n_wave_groups = hg.n_list;
    out->last_ms = ms; out->resolve_ms = resolve_ms;
  }
  return 0;
}
