// kamd_ixbuild.hip -- the k-mer table built on the device: kamd_index_upload on an index loaded with kamd_index_load_deferred, and
// kamd_ctx_table_info / kamd_ctx_table_download.
//
// The host builder (kamd_index.cpp) enumerates all k-mers twice, writes gigabytes at random into host memory and copies them across the
// link.  Here only the unitig text and the block tables cross it; the table is rebuilt from them:
//   k_ixb_count   one lane per text position: is it a k-mer start, which home bucket
//   scan          base[b] = max(end[b-1], b*S), end[b] = base[b] + fill[b] as a three-launch scan of max-plus maps (per-block reduce, scan of
//                 the block summaries, apply) with max_disp and end_cursor beside it; ONE read-back per round, then the host's geometry
//                 decision (kamd_ixbuild.h), which may enlarge the table and repeat count + scan
//   k_ixb_place   slot = base[hb] + atomicAdd(fill2[hb]); only the text position is staged
//   k_ixb_order   the staged positions of every home group ascending: what ONE host thread lays down, whatever the atomics' order was
//   k_ixb_fill    one lane per slot: the slot's words, slot_block, slot_dist from the staged position alone
// The D-list table goes through the same kernels with its (sorted, distinct) keys in place of the text; the dummy hit is a probe of the
// finished table.  The per-item steps are the host/device functions of kamd_ixbuild.h.  No kernel waits for another workgroup.
#include "kamd_dev.h"
#include "kamd_ixbuild.h"

namespace ixb = kamd::ixb;

namespace {
constexpr int SCAN_PER_THREAD = 8, SCAN_CHUNK = BLOCK * SCAN_PER_THREAD;   // buckets per thread / per workgroup of the scan

// items: text positions [0, text_bases), or (keys != null) the keys of the D-list
__global__ void k_ixb_count(ixb::TextView t, const uint64_t* __restrict__ keys, uint64_t n_items, uint64_t nb, u32* fill) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_items) return;
  uint64_t hb;
  if (keys) hb = kamd::home_bucket(keys[i], nb);
  else {
    // the unitig of the wavefront's first position by binary search (the same words for all lanes), then forward
    const uint64_t u = ixb::unitig_from(t, ixb::unitig_of(t, i & ~(uint64_t)63), i);
    if (!ixb::kmer_home(t, u, i, nb, &hb)) return;
  }
  if (hb < nb) atomicAdd(&fill[hb], 1u);
}
__global__ void k_ixb_place(ixb::TextView t, const uint64_t* __restrict__ keys, uint64_t n_items, uint64_t nb, const uint64_t* __restrict__ base, u32* fill2,
                            u32* staged, uint64_t total_slots) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_items) return;
  uint64_t hb;
  if (keys) hb = kamd::home_bucket(keys[i], nb);
  else {
    const uint64_t u = ixb::unitig_from(t, ixb::unitig_of(t, i & ~(uint64_t)63), i);
    if (!ixb::kmer_home(t, u, i, nb, &hb)) return;
  }
  if (hb >= nb) return;
  const uint64_t slot = base[hb] + atomicAdd(&fill2[hb], 1u);
  if (slot < total_slots) staged[slot] = (u32)i;
}
__global__ void k_ixb_order(const u32* __restrict__ fill, const uint64_t* __restrict__ base, uint64_t nb, u32* staged, uint64_t total_slots) {
  const uint64_t b = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= nb) return;
  const u32 n = fill[b];
  if (n < 2 || base[b] + n > total_slots) return;
  ixb::order_group(staged + base[b], n);
}
__global__ void k_ixb_fill(ixb::FillView f, const u32* __restrict__ staged, uint64_t total_slots, uint64_t* table, u32* slot_block, u32* slot_dist) {
  const uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= total_slots) return;
  ixb::fill_slot(f, s, staged[s], table, slot_block, slot_dist);
}

// ---- the scan: no workgroup waits for another one ----
__device__ __forceinline__ ixb::ScanOp thread_op(const u32* fill, uint64_t nb, u32 S, uint64_t b0) {
  ixb::ScanOp op = ixb::scan_identity();
  for (int i = 0; i < SCAN_PER_THREAD; i++) if (b0 + i < nb) op = ixb::scan_compose(op, ixb::scan_op_of(fill[b0 + i], S));
  return op;
}
// inclusive scan of the workgroup's maps in thread order; returns the map of the threads BEFORE this one
__device__ __forceinline__ ixb::ScanOp block_exclusive(ixb::ScanOp op, ixb::ScanOp* lds, ixb::ScanOp* total) {
  const int t = threadIdx.x;
  lds[t] = op;
  __syncthreads();
  for (int d = 1; d < BLOCK; d <<= 1) {
    ixb::ScanOp v = lds[t];
    if (t >= d) v = ixb::scan_compose(lds[t - d], v);
    __syncthreads();
    lds[t] = v;
    __syncthreads();
  }
  const ixb::ScanOp ex = t ? lds[t - 1] : ixb::scan_identity();
  if (total) *total = lds[BLOCK - 1];
  return ex;
}
__global__ void __launch_bounds__(BLOCK) k_ixb_scan_reduce(const u32* __restrict__ fill, uint64_t nb, u32 S, ixb::ScanOp* sums) {
  __shared__ ixb::ScanOp lds[BLOCK];
  ixb::ScanOp total;
  (void)block_exclusive(thread_op(fill, nb, S, (uint64_t)blockIdx.x * SCAN_CHUNK + (uint64_t)threadIdx.x * SCAN_PER_THREAD), lds, &total);
  if (threadIdx.x == 0) sums[blockIdx.x] = total;
}
// one workgroup: x that enters every chunk
__global__ void __launch_bounds__(BLOCK) k_ixb_scan_sums(const ixb::ScanOp* __restrict__ sums, uint64_t n_chunks, long long* xin) {
  __shared__ ixb::ScanOp lds[BLOCK];
  const uint64_t per = (n_chunks + BLOCK - 1) / BLOCK;
  const uint64_t a = std::min<uint64_t>(n_chunks, per * threadIdx.x), e = std::min<uint64_t>(n_chunks, a + per);
  ixb::ScanOp op = ixb::scan_identity();
  for (uint64_t i = a; i < e; i++) op = ixb::scan_compose(op, sums[i]);
  const ixb::ScanOp ex = block_exclusive(op, lds, nullptr);
  int64_t x = ixb::scan_apply(ex, 0);
  for (uint64_t i = a; i < e; i++) { xin[i] = x; x = ixb::scan_apply(sums[i], x); }
}
// out[0] = end_cursor, out[1] = max_disp (zeroed by the host)
__global__ void __launch_bounds__(BLOCK) k_ixb_scan_apply(const u32* __restrict__ fill, uint64_t nb, u32 S, const long long* __restrict__ xin, uint64_t* base, uint64_t* out) {
  __shared__ ixb::ScanOp lds[BLOCK];
  __shared__ uint64_t red[BLOCK];
  const uint64_t b0 = (uint64_t)blockIdx.x * SCAN_CHUNK + (uint64_t)threadIdx.x * SCAN_PER_THREAD;
  const ixb::ScanOp ex = block_exclusive(thread_op(fill, nb, S, b0), lds, nullptr);
  int64_t x = ixb::scan_apply(ex, xin[blockIdx.x]);
  uint64_t md = 0;
  for (int i = 0; i < SCAN_PER_THREAD; i++) {
    const uint64_t b = b0 + i;
    if (b >= nb) break;
    const u32 n = fill[b];
    const ixb::ScanOut o = ixb::scan_bucket(x, b, n, S);
    base[b] = o.base;
    if (n) md = std::max<uint64_t>(md, ixb::bucket_disp(o.end, b, S));
    if (b + 1 == nb) out[0] = o.end;
  }
  red[threadIdx.x] = md;
  __syncthreads();
  for (int d = BLOCK / 2; d > 0; d >>= 1) { if ((int)threadIdx.x < d) red[threadIdx.x] = std::max(red[threadIdx.x], red[threadIdx.x + d]); __syncthreads(); }
  if (threadIdx.x == 0 && red[0]) atomicMax((unsigned long long*)&out[1], (unsigned long long)red[0]);
}

// the dummy hit (um_dummy = dbg.find(first D-list k-mer), KmerIndex.cpp:1386-1403): out = {found, slot, uec, strand}
__global__ void k_ixb_dummy(kamd::Table t, uint64_t key, uint64_t* out) {
  if (blockIdx.x || threadIdx.x) return;
  const kamd::Probe p = kamd::probe_table(t, key, true, nullptr);
  out[0] = p.found ? 1 : 0; out[1] = p.slot; out[2] = p.uec; out[3] = p.strand ? 1 : 0;
}

// device memory of one build: freed when the build returns, however it returns
struct Scratch {
  hipStream_t s; std::vector<void*> p;
  explicit Scratch(hipStream_t st) : s(st) {}
  ~Scratch() { if (!p.empty()) (void)hipStreamSynchronize(s); for (void* q : p) (void)hipFree(q); }
  template <class T> int get(size_t n, T** out) {
    void* q = nullptr;
    HIPC(hipMalloc(&q, std::max<size_t>(n, 1) * sizeof(T)));
    p.push_back(q); *out = (T*)q;
    return 0;
  }
  void drop(void* q) { auto it = std::find(p.begin(), p.end(), q); if (it != p.end()) { (void)hipStreamSynchronize(s); (void)hipFree(q); p.erase(it); } }
};
struct Timer {
  hipEvent_t a = nullptr, b = nullptr; hipStream_t s;
  explicit Timer(hipStream_t st) : s(st) { (void)hipEventCreate(&a); (void)hipEventCreate(&b); }
  ~Timer() { if (a) (void)hipEventDestroy(a); if (b) (void)hipEventDestroy(b); }
  void start() { (void)hipEventRecord(a, s); }
  float stop() { float ms = 0.f; if (hipEventRecord(b, s) != hipSuccess || hipEventSynchronize(b) != hipSuccess || hipEventElapsedTime(&ms, a, b) != hipSuccess) return 0.f; return ms; }
};

// count + scan for a table of nb home buckets: fill[nb + 1], base[nb] (both allocated by the caller), end_cursor and max_disp read back
int count_and_scan(kamd_ctx* c, Scratch& sc, const ixb::TextView& tv, const uint64_t* keys, uint64_t n_items, uint64_t nb, u32 S, u32* fill, uint64_t* base, uint64_t* end_cursor, uint64_t* max_disp) {
  HIPC(hipMemsetAsync(fill, 0, (nb + 1) * sizeof(u32), c->stream));
  if (n_items) hipLaunchKernelGGL(k_ixb_count, dim3(grid_for(n_items, BLOCK)), dim3(BLOCK), 0, c->stream, tv, keys, n_items, nb, fill);
  const uint64_t n_chunks = (nb + SCAN_CHUNK - 1) / SCAN_CHUNK;
  ixb::ScanOp* sums = nullptr; long long* xin = nullptr; uint64_t* out = nullptr;
  if (int rc = sc.get(n_chunks, &sums)) return rc;
  if (int rc = sc.get(n_chunks, &xin)) return rc;
  if (int rc = sc.get(2, &out)) return rc;
  HIPC(hipMemsetAsync(out, 0, 2 * sizeof(uint64_t), c->stream));
  hipLaunchKernelGGL(k_ixb_scan_reduce, dim3((unsigned)n_chunks), dim3(BLOCK), 0, c->stream, fill, nb, S, sums);
  hipLaunchKernelGGL(k_ixb_scan_sums, dim3(1), dim3(BLOCK), 0, c->stream, sums, n_chunks, xin);
  hipLaunchKernelGGL(k_ixb_scan_apply, dim3((unsigned)n_chunks), dim3(BLOCK), 0, c->stream, fill, nb, S, xin, base, out);
  HIPC(hipGetLastError());
  uint64_t host[2] = {0, 0};
  HIPC(hipMemcpyAsync(host, out, sizeof host, hipMemcpyDeviceToHost, c->stream));
  HIPC(hipStreamSynchronize(c->stream));
  *end_cursor = host[0]; *max_disp = host[1];
  sc.drop(sums); sc.drop(xin); sc.drop(out);
  return 0;
}
// place + order + fill into `table` (total_buckets lines) and, for the k-mer table, slot_block / slot_dist
int place_order_fill(kamd_ctx* c, Scratch& sc, ixb::FillView f, uint64_t n_items, u32* fill, uint64_t* table, u32* slot_block, u32* slot_dist, float* ms3) {
  const uint64_t total_slots = f.total_buckets * f.S;
  u32* staged = nullptr;
  if (int rc = sc.get(total_slots, &staged)) return rc;
  Timer tm(c->stream);
  tm.start();
  HIPC(hipMemsetAsync(staged, 0xFF, total_slots * sizeof(u32), c->stream));
  // (the counters of the placement: the counts are kept for the ordering)
  u32* fill2 = nullptr;
  if (int rc = sc.get(f.nb + 1, &fill2)) return rc;
  HIPC(hipMemsetAsync(fill2, 0, (f.nb + 1) * sizeof(u32), c->stream));
  if (n_items) hipLaunchKernelGGL(k_ixb_place, dim3(grid_for(n_items, BLOCK)), dim3(BLOCK), 0, c->stream, f.text, f.keys, n_items, f.nb, f.base, fill2, staged, total_slots);
  HIPC(hipGetLastError());
  ms3[0] = tm.stop();
  tm.start();
  hipLaunchKernelGGL(k_ixb_order, dim3(grid_for(f.nb, BLOCK)), dim3(BLOCK), 0, c->stream, fill, f.base, f.nb, staged, total_slots);
  HIPC(hipGetLastError());
  ms3[1] = tm.stop();
  tm.start();
  hipLaunchKernelGGL(k_ixb_fill, dim3(grid_for(total_slots, BLOCK)), dim3(BLOCK), 0, c->stream, f, staged, total_slots, table, slot_block, slot_dist);
  HIPC(hipGetLastError());
  ms3[2] = tm.stop();
  sc.drop(staged); sc.drop(fill2);
  return 0;
}
template <class T> int index_alloc(kamd_ctx* c, size_t n, T** out) {
  void* p = nullptr;
  HIPC(hipMalloc(&p, std::max<size_t>(n, 1) * sizeof(T)));
  c->index_allocs.push_back(p);
  *out = (T*)p;
  return 0;
}
}  // namespace

namespace kamdi {
// d: the device index as far as kamd_index_upload has filled it (utext, the block tables); on return its table fields are set
int index_build_device(kamd_ctx* c, const kamd_index* hix, const kamd_index_view& v, DevIndex* d, kamd_table_info* info) {
  kamd_ixbuild_info bi;
  if (int rc = kamd_ixbuild_info_get(hix, &bi)) return rc;
  if (v.text_bases >= 0xFFFFFF00ULL || v.n_blocks >= 0xFFFFFFFFULL) return kamd::fail(-3, "index: too large for the device builder");
  Scratch sc(c->stream);
  Timer whole(c->stream), part(c->stream);
  whole.start();
  // what only the build reads: where the unitigs start in the text, the blocks' classes
  uint64_t* d_gpos = nullptr; u32* d_blk_uec = nullptr;
  if (int rc = sc.get(v.n_unitigs + 1, &d_gpos)) return rc;
  if (int rc = sc.get(v.n_blocks, &d_blk_uec)) return rc;
  HIPC(hipMemcpyAsync(d_gpos, v.unitig_gpos, (v.n_unitigs + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, c->stream));
  if (v.n_blocks) HIPC(hipMemcpyAsync(d_blk_uec, bi.blk_uec, v.n_blocks * sizeof(u32), hipMemcpyHostToDevice, c->stream));
  const ixb::TextView tv{d->utext, d_gpos, v.n_unitigs, v.text_bases, v.k};

  ixb::Geometry geo;
  if (!ixb::geometry_init(geo, v.k, v.n_kmers, bi.layout, bi.load)) return kamd::fail(-3, "index: too many k-mers for 32-bit bucket numbers");
  u32* fill = nullptr; uint64_t* base = nullptr; uint64_t have_nb = 0;
  uint64_t end_cursor = 0, max_disp = 0;
  int rounds = 0;
  part.start();
  for (;;) {
    const int fit = ixb::geometry_fit(geo, v.n_uec, v.text_bases);
    if (fit == ixb::GEO_FAIL) return kamd::fail(-3, "index: the compact k-mer table cannot hold this index (class ids / text positions too wide); use KAMD_TABLE_LAYOUT=wide or auto");
    if (geo.nb > have_nb) {
      if (fill) { sc.drop(fill); sc.drop(base); }
      if (int rc = sc.get(geo.nb + 1, &fill)) return rc;
      if (int rc = sc.get(geo.nb, &base)) return rc;
      have_nb = geo.nb;
    }
    if (int rc = count_and_scan(c, sc, tv, nullptr, v.text_bases, geo.nb, (u32)geo.S, fill, base, &end_cursor, &max_disp)) return rc;
    ++rounds;
    if (ixb::geometry_after_scan(geo, max_disp) == ixb::GEO_OK) break;
    if (geo.nb >= 0xF0000000ULL) return kamd::fail(-3, "index: too many k-mers for 32-bit bucket numbers");
  }
  info->build_count_ms = part.stop();
  const uint64_t nb = geo.nb, S = geo.S, total_buckets = ixb::total_buckets_of(nb, end_cursor, S);
  uint64_t* table = nullptr; u32* slot_block = nullptr; u32* slot_dist = nullptr;
  if (int rc = index_alloc(c, total_buckets * 8, &table)) return rc;
  if (int rc = index_alloc(c, total_buckets * S, &slot_block)) return rc;
  if (int rc = index_alloc(c, total_buckets * S, &slot_dist)) return rc;
  ixb::FillView f{};
  f.text = tv; f.unitig_blk_off = (const uint64_t*)d->unitig_blk_off; f.blk_lb = d->blk_lb; f.blk_ub = d->blk_ub; f.blk_uec = d_blk_uec; f.n_blocks = v.n_blocks;
  f.base = (const uint64_t*)base; f.nb = nb; f.total_buckets = total_buckets; f.end_cursor = end_cursor;
  f.S = (u32)S; f.layout = geo.compact ? kamd::LAYOUT_COMPACT : kamd::LAYOUT_WIDE;
  f.tag_q = geo.compact ? geo.tag_q : 0; f.tag_dsh = geo.compact ? geo.tag_dsh : 0; f.tag_w = geo.compact ? geo.tag_w : 0;
  f.keys = nullptr; f.n_keys = 0;
  float ms3[3] = {0.f, 0.f, 0.f};
  if (int rc = place_order_fill(c, sc, f, v.text_bases, fill, (uint64_t*)table, slot_block, slot_dist, ms3)) return rc;
  info->build_place_ms = ms3[0]; info->build_order_ms = ms3[1]; info->build_fill_ms = ms3[2];
  sc.drop(fill); sc.drop(base);
  d->table = (const u64*)table; d->n_buckets = nb; d->slot_block = slot_block; d->slot_dist = slot_dist;
  d->table_layout = (int)f.layout; d->tag_q = f.tag_q; d->tag_dsh = f.tag_dsh; d->tag_w = f.tag_w;
  info->n_buckets = nb; info->pad_buckets = total_buckets - nb; info->table_layout = f.layout; info->slots_per_bucket = (u32)S;
  info->tag_q = f.tag_q; info->tag_dsh = f.tag_dsh; info->tag_w = f.tag_w; info->build_rounds = rounds;

  // ---- D-list table (always wide) and the dummy hit ----
  d->dtable = nullptr; d->n_dbuckets = 0; d->dummy_slot = 0; d->dummy_uec = 0; d->dummy_strand = 0;
  info->n_dbuckets = info->dpad_buckets = 0; info->dummy_slot = 0; info->dummy_uec = info->dummy_strand = 0;
  part.start();
  if (v.dlist_size) {
    std::vector<uint64_t> keys(bi.dlist_keys, bi.dlist_keys + v.dlist_size);
    std::sort(keys.begin(), keys.end());
    keys.erase(std::unique(keys.begin(), keys.end()), keys.end());
    const uint64_t nk = keys.size(), ndb = ixb::dlist_home_buckets(v.dlist_size);
    uint64_t* d_keys = nullptr; u32* dfill = nullptr; uint64_t* dbase = nullptr;
    if (int rc = sc.get(nk, &d_keys)) return rc;
    if (int rc = sc.get(ndb + 1, &dfill)) return rc;
    if (int rc = sc.get(ndb, &dbase)) return rc;
    HIPC(hipMemcpyAsync(d_keys, keys.data(), nk * sizeof(uint64_t), hipMemcpyHostToDevice, c->stream));
    uint64_t dend = 0, ddisp = 0;
    if (int rc = count_and_scan(c, sc, tv, (const uint64_t*)d_keys, nk, ndb, kamd::BUCKET_SLOTS, dfill, dbase, &dend, &ddisp)) return rc;   // (synchronises: `keys` has crossed)
    const uint64_t tb = ixb::total_buckets_of(ndb, dend, kamd::BUCKET_SLOTS);
    uint64_t* dtable = nullptr;
    if (int rc = index_alloc(c, tb * 8, &dtable)) return rc;
    ixb::FillView g{};
    g.text = tv; g.base = (const uint64_t*)dbase; g.nb = ndb; g.total_buckets = tb; g.end_cursor = dend; g.S = kamd::BUCKET_SLOTS; g.layout = kamd::LAYOUT_WIDE;
    g.keys = (const uint64_t*)d_keys; g.n_keys = nk;
    float dms[3];
    if (int rc = place_order_fill(c, sc, g, nk, dfill, (uint64_t*)dtable, nullptr, nullptr, dms)) return rc;
    d->dtable = (const u64*)dtable; d->n_dbuckets = ndb;
    info->n_dbuckets = ndb; info->dpad_buckets = tb - ndb;
    // the dummy: the first D-list k-mer looked up in the finished table
    uint64_t* d_out = nullptr;
    if (int rc = sc.get(4, &d_out)) return rc;
    HIPC(hipMemsetAsync(d_out, 0, 4 * sizeof(uint64_t), c->stream));
    hipLaunchKernelGGL(k_ixb_dummy, dim3(1), dim3(64), 0, c->stream, make_table(*d, false), (uint64_t)bi.dlist_keys[0], d_out);
    HIPC(hipGetLastError());
    uint64_t out[4] = {0, 0, 0, 0};
    HIPC(hipMemcpyAsync(out, d_out, sizeof out, hipMemcpyDeviceToHost, c->stream));
    HIPC(hipStreamSynchronize(c->stream));
    if (!out[0]) return kamd::fail(-3, "index: Dummy k-mer not found in graph");   // KmerIndex.cpp:1398-1401
    d->dummy_slot = out[1]; d->dummy_uec = (u32)out[2]; d->dummy_strand = (u32)out[3];
    info->dummy_slot = out[1]; info->dummy_uec = (u32)out[2]; info->dummy_strand = (u32)out[3];
  }
  info->build_dlist_ms = part.stop();
  info->built_on_device = 1;
  info->build_ms = whole.stop();
  return 0;
}
}  // namespace kamdi

extern "C" int kamd_ctx_table_info(kamd_ctx* c, kamd_table_info* out) {
  if (!c || !out) return kamd::fail(-1, "kamd_ctx_table_info: null argument");
  if (!c->has_index) return kamd::fail(-1, "kamd_ctx_table_info: no index uploaded");
  *out = c->tinfo;
  return 0;
}
extern "C" int kamd_ctx_table_download(kamd_ctx* c, uint64_t* table, uint32_t* slot_block, uint32_t* slot_dist, uint64_t* dtable) {
  if (!c) return kamd::fail(-1, "kamd_ctx_table_download: null argument");
  if (!c->has_index) return kamd::fail(-1, "kamd_ctx_table_download: no index uploaded");
  HIPC(hipSetDevice(c->device));
  const kamd_table_info& t = c->tinfo;
  const size_t lines = (size_t)(t.n_buckets + t.pad_buckets), slots = lines * t.slots_per_bucket, dlines = (size_t)(t.n_dbuckets + t.dpad_buckets);
  if (table && lines) HIPC(hipMemcpyAsync(table, c->ix.table, lines * 8 * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
  if (slot_block && slots) HIPC(hipMemcpyAsync(slot_block, c->ix.slot_block, slots * sizeof(u32), hipMemcpyDeviceToHost, c->stream));
  if (slot_dist && slots) HIPC(hipMemcpyAsync(slot_dist, c->ix.slot_dist, slots * sizeof(u32), hipMemcpyDeviceToHost, c->stream));
  if (dtable && dlines && c->ix.dtable) HIPC(hipMemcpyAsync(dtable, c->ix.dtable, dlines * 8 * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
  HIPC(hipStreamSynchronize(c->stream));
  return 0;
}
