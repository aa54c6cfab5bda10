// kamd_inflate.hip -- BGZF members inflated on the device, and the line arithmetic the FASTQ front-end needs on a text that never was on the host.
//   k_bgzf_inflate   one wavefront (a workgroup of 64) per member, a grid of members; nobody waits for anybody.  The member's whole text (at most
//                    64 KiB) stays in LDS until it is complete and its CRC-32 agrees, so a back-reference never reads global memory this kernel
//                    wrote, and a corrupt member writes nothing.  LDS per wavefront: 64 KiB + 16 of text, 6.5 KiB of tables and queues
//                    (kamd_inflate.h Work) = 72 KiB, i.e. two wavefronts per CU of 160 KiB -- what a unit of some 500 members fills anyway.
//                    The text lies in LDS at its destination's offset within 16 bytes, so the flush is aligned 16-byte loads and stores
//                    whatever the destination offset; the compressed bytes are read as aligned dwords into a 64-bit bit buffer.
//                    The CRC-32 runs in the same kernel over the text in LDS: a slice per lane, combined by x^(8 len) mod P; the same pass
//                    counts the member's newlines.
//   k_text_lines     newlines of a device text per chunk of TEXT_CHUNK bytes (one wavefront per chunk, 16-byte loads)
//   k_text_locate    one wavefront: the texts' line totals from the chunk counts, the number of whole records, and for every text the offset
//                    just behind line 4 * records (the chunk by a scan of the counts, then a search inside the chunk)
// The decoder, the CRC and the per-range line functions live in kamd_inflate.h (shared with the CPU build of tests/emu_inflate).
#include "kamd_dev.h"
#include "kamd_inflate.h"

namespace {
using namespace kamd::inf;

struct MemberRes { int32_t reason; u32 newlines; };
constexpr int INF_BLOCK = 64;   // ONE wavefront per member: the decoder's redundant stores are races with more (kamd_inflate.h)
static_assert(INF_BLOCK == LANES, "k_bgzf_inflate: the shared decoder is written for the lockstep lanes of a single wavefront");

// CRC = false (kamd_debug_bgzf_inflate only): the text is flushed unchecked and no newlines are counted -- what the check costs is the difference
template <bool CRC>
__global__ __launch_bounds__(INF_BLOCK) void k_bgzf_inflate(const uint8_t* __restrict__ comp, const kamd_bgzf_member* __restrict__ members, u64 n_members,
                                                            uint8_t* text, MemberRes* res) {
  __shared__ __attribute__((aligned(16))) uint8_t s_out[MAX_ISIZE + 16];
  __shared__ Work s_w;
  const u64 m = blockIdx.x;
  if (m >= n_members) return;
  const int lane = (int)threadIdx.x;
  const kamd_bgzf_member mb = members[m];
  uint8_t* g = text + mb.dst_off;
  const u32 a = (u32)((uintptr_t)g & 15);
  uint8_t* out = s_out + a;   // LDS and destination agree mod 16
  crc_table_fill(s_w.crc_tab, lane, INF_BLOCK);
  int r = inflate_member(comp + mb.src_off, mb.src_len, out, mb.isize, s_w, lane, INF_BLOCK, [] { __syncthreads(); });
  u32 nl = 0;
  if (CRC && !r) {
    __syncthreads();
    u32 term = crc_slice_term(out, mb.isize, s_w.crc_tab, lane, INF_BLOCK, &nl);
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) { term ^= (u32)__shfl_xor((int)term, d, 64); nl += (u32)__shfl_xor((int)nl, d, 64); }
    if (~term != mb.crc32) r = INF_CRC;
  }
  if (!r) {
    const u32 x0 = a, x1 = a + mb.isize, body0 = (x0 + 15u) & ~15u, body1 = x1 & ~15u;
    uint8_t* gb = g - a;
    if (body0 >= body1) {
      for (u32 x = x0 + (u32)lane; x < x1; x += INF_BLOCK) gb[x] = s_out[x];
    } else {
      if (x0 + (u32)lane < body0) gb[x0 + lane] = s_out[x0 + lane];
      for (u32 x = body0 + 16u * (u32)lane; x < body1; x += 16u * INF_BLOCK) *reinterpret_cast<uint4*>(gb + x) = *reinterpret_cast<const uint4*>(s_out + x);
      if (body1 + (u32)lane < x1) gb[body1 + lane] = s_out[body1 + lane];
    }
  }
  if (lane == 0) res[m] = MemberRes{r, r ? 0u : nl};
}

__global__ __launch_bounds__(64) void k_text_lines(const uint8_t* __restrict__ t, u64 n, u32* __restrict__ counts) {
  const u64 lo = (u64)blockIdx.x * TEXT_CHUNK, hi = min(n, lo + TEXT_CHUNK);
  const int lane = lane_id();
  u64 cnt = 0;
  for (u64 x = lo + 16ull * (u64)lane; x < hi; x += 16ull * 64) {
    const uint4 v = *reinterpret_cast<const uint4*>(t + x);   // (t is 16-byte aligned and readable behind n: kamd_text_cut)
    const u32 w[4] = {v.x, v.y, v.z, v.w};
    const u64 valid = hi - x;
#pragma unroll
    for (int j = 0; j < 4; j++) {
      u32 q = w[j];
      if (valid < 4ull * j + 4) q = valid <= 4ull * j ? 0u : q & ((1u << (8 * (u32)(valid - 4ull * j))) - 1u);   // (a zero byte is no newline)
      cnt += nl_count32(q);
    }
  }
  cnt = wave_sum64(cnt);
  if (lane == 0) counts[blockIdx.x] = (u32)cnt;
}

struct CutArgs { const uint8_t* t[2]; u64 n[2]; const u32* counts[2]; u64 nc[2]; int n_files; u64 max_records; };

// out[0] = records, out[1 + f] = end of text f
__global__ __launch_bounds__(64) void k_text_locate(CutArgs a, u64* out) {
  const int lane = lane_id();
  uint64_t lines[2] = {0, 0};
  for (int f = 0; f < a.n_files; f++) {
    u64 s = 0;
    for (u64 c = (u64)lane; c < a.nc[f]; c += 64) s += a.counts[f][c];
    lines[f] = shfl_u64(wave_sum64(s), 0);
  }
  const u64 R = records_of(lines, a.n_files, a.max_records), k = 4 * R;
  if (lane == 0) out[0] = R;
  for (int f = 0; f < a.n_files; f++) {
    if (k == 0) { if (lane == 0) out[1 + f] = 0; continue; }
    // the chunk that holds newline k (lines[f] >= k: there is one), and the newline's number inside it
    u64 before = 0, chunk = 0, r = 0;
    for (u64 g = 0; g * 64 < a.nc[f]; g++) {
      const u64 c = g * 64 + (u64)lane;
      const u32 v = c < a.nc[f] ? a.counts[f][c] : 0u;
      const u32 incl = wave_incl_scan(v);
      const u32 tot = (u32)__shfl((int)incl, 63, 64);
      if (before + tot >= k) {
        const bool mine = before + incl >= k && before + incl - v < k;
        const int src = __ffsll((unsigned long long)__ballot(mine)) - 1;
        chunk = g * 64 + (u64)src;
        r = shfl_u64(k - (before + incl - v), src);
        break;
      }
      before += tot;
    }
    const u64 lo = chunk * TEXT_CHUNK, hi = min(a.n[f], lo + TEXT_CHUNK);
    const u64 plo = min(hi, lo + (u64)lane * (TEXT_CHUNK / 64)), phi = min(hi, plo + TEXT_CHUNK / 64);
    const u32 pc = (u32)lines_range(a.t[f], plo, phi);
    const u32 incl = wave_incl_scan(pc);
    if (incl >= r && incl - pc < r) out[1 + f] = locate_in(a.t[f], plo, phi, r - (incl - pc));
  }
}

}  // namespace

namespace {
int bgzf_inflate_impl(kamd_ctx* c, const uint8_t* d_comp, uint64_t comp_bytes, const kamd_bgzf_member* members, uint64_t n_members, char* d_text,
                      uint64_t text_cap, kamd_inflate_result* out, bool check_crc, float* kernel_ms, const char* who) {
  const std::string w(who);
  if (!c || !out) return kamd::fail(-1, w + ": null argument");
  *out = kamd_inflate_result{};
  if (kernel_ms) *kernel_ms = 0.f;
  if (n_members == 0) return 0;
  if (!d_comp || !members || !d_text) return kamd::fail(-1, w + ": null argument");
  if ((uintptr_t)d_comp & 3) return kamd::fail(-1, w + ": d_comp must be 4-byte aligned (the members' offsets are arbitrary)");
  if (n_members >= 0x7FFFFFFFULL) return kamd::fail(-1, w + ": too many members for one launch");
  u64 n_bytes = 0;
  for (u64 i = 0; i < n_members; i++) {
    const kamd_bgzf_member& m = members[i];
    if (m.src_off > comp_bytes || m.src_len > comp_bytes - m.src_off)
      return kamd::fail(-1, w + ": member " + std::to_string(i) + " reads beyond comp_bytes");
    if (m.src_len > MAX_SRC_LEN) return kamd::fail(-1, w + ": member " + std::to_string(i) + " has a stream of more than 1 MiB (src_len)");
    if (m.isize > MAX_ISIZE) return kamd::fail(-1, w + ": member " + std::to_string(i) + " holds more than 65536 bytes of text");
    if (m.dst_off > text_cap || m.isize > text_cap - m.dst_off)
      return kamd::fail(-1, w + ": member " + std::to_string(i) + " writes beyond text_cap");
    n_bytes += m.isize;
  }
  HIPC(hipSetDevice(c->device));
  if (int rc = c->inf_members.ensure(n_members * sizeof(kamd_bgzf_member), 0, c->stream)) return rc;
  if (int rc = c->inf_res.ensure(n_members * sizeof(MemberRes), 0, c->stream)) return rc;
  if (kernel_ms) for (hipEvent_t* e : {&c->ev0, &c->ev1}) if (!*e) HIPC(hipEventCreate(e));
  HIPC(hipMemcpyAsync(c->inf_members.p, members, n_members * sizeof(kamd_bgzf_member), hipMemcpyHostToDevice, c->stream));
  if (kernel_ms) HIPC(hipEventRecord(c->ev0, c->stream));
  const kamd_bgzf_member* dm = c->inf_members.as<kamd_bgzf_member>();
  if (check_crc) hipLaunchKernelGGL(k_bgzf_inflate<true>, dim3((unsigned)n_members), dim3(INF_BLOCK), 0, c->stream, d_comp, dm, (u64)n_members, reinterpret_cast<uint8_t*>(d_text), c->inf_res.as<MemberRes>());
  else hipLaunchKernelGGL(k_bgzf_inflate<false>, dim3((unsigned)n_members), dim3(INF_BLOCK), 0, c->stream, d_comp, dm, (u64)n_members, reinterpret_cast<uint8_t*>(d_text), c->inf_res.as<MemberRes>());
  HIPC(hipGetLastError());
  if (kernel_ms) HIPC(hipEventRecord(c->ev1, c->stream));
  std::vector<MemberRes> res(n_members);
  HIPC(hipMemcpyAsync(res.data(), c->inf_res.p, n_members * sizeof(MemberRes), hipMemcpyDeviceToHost, c->stream));
  HIPC(hipStreamSynchronize(c->stream));
  if (kernel_ms) HIPC(hipEventElapsedTime(kernel_ms, c->ev0, c->ev1));
  out->n_bytes = n_bytes;
  for (u64 i = 0; i < n_members; i++) {
    if (res[i].reason) { out->status = 1; out->reason = res[i].reason; out->first_bad_member = i; out->n_newlines = 0; return 0; }
    out->n_newlines += res[i].newlines;
  }
  return 0;
}
}  // namespace

extern "C" int kamd_bgzf_inflate(kamd_ctx* c, const uint8_t* d_comp, uint64_t comp_bytes, const kamd_bgzf_member* members, uint64_t n_members, char* d_text,
                                 uint64_t text_cap, kamd_inflate_result* out) {
  return bgzf_inflate_impl(c, d_comp, comp_bytes, members, n_members, d_text, text_cap, out, true, nullptr, "kamd_bgzf_inflate");
}
extern "C" int kamd_debug_bgzf_inflate(kamd_ctx* c, const uint8_t* d_comp, uint64_t comp_bytes, const kamd_bgzf_member* members, uint64_t n_members, char* d_text,
                                       uint64_t text_cap, int32_t check_crc, kamd_inflate_result* out, float* kernel_ms) {
  return bgzf_inflate_impl(c, d_comp, comp_bytes, members, n_members, d_text, text_cap, out, check_crc != 0, kernel_ms, "kamd_debug_bgzf_inflate");
}

extern "C" int kamd_text_cut(kamd_ctx* c, const char* const* d_text, const uint64_t* n_bytes, int32_t n_files, uint64_t max_records, uint64_t* n_records,
                             uint64_t* end) {
  if (!c || !d_text || !n_bytes || !n_records || !end) return kamd::fail(-1, "kamd_text_cut: null argument");
  if (n_files < 1 || n_files > 2) return kamd::fail(-1, "kamd_text_cut: n_files must be 1 or 2");
  CutArgs a{};
  a.n_files = n_files; a.max_records = max_records;
  u64 nc_total = 0;
  for (int f = 0; f < n_files; f++) {
    if (n_bytes[f] && !d_text[f]) return kamd::fail(-1, "kamd_text_cut: null text");
    if ((uintptr_t)d_text[f] & 15) return kamd::fail(-1, "kamd_text_cut: the text must be 16-byte aligned");
    a.t[f] = reinterpret_cast<const uint8_t*>(d_text[f]); a.n[f] = n_bytes[f];
    a.nc[f] = (n_bytes[f] + TEXT_CHUNK - 1) / TEXT_CHUNK;
    if (a.nc[f] >= 0x7FFFFFFFULL) return kamd::fail(-1, "kamd_text_cut: text too large for one launch");
    nc_total += a.nc[f];
  }
  HIPC(hipSetDevice(c->device));
  if (int rc = c->txt_counts.ensure(std::max<u64>(nc_total, 1) * sizeof(u32), 0, c->stream)) return rc;
  if (int rc = c->txt_res.ensure(3 * sizeof(u64), 0, c->stream)) return rc;
  u32* counts = c->txt_counts.as<u32>();
  for (int f = 0; f < n_files; f++) {
    a.counts[f] = counts;
    if (a.nc[f]) {
      hipLaunchKernelGGL(k_text_lines, dim3((unsigned)a.nc[f]), dim3(64), 0, c->stream, a.t[f], a.n[f], counts);
      HIPC(hipGetLastError());
    }
    counts += a.nc[f];
  }
  hipLaunchKernelGGL(k_text_locate, dim3(1), dim3(64), 0, c->stream, a, c->txt_res.as<u64>());
  HIPC(hipGetLastError());
  u64 h[3] = {0, 0, 0};
  HIPC(hipMemcpyAsync(h, c->txt_res.p, sizeof h, hipMemcpyDeviceToHost, c->stream));
  HIPC(hipStreamSynchronize(c->stream));
  *n_records = h[0];
  for (int f = 0; f < n_files; f++) end[f] = h[1 + f];
  return 0;
}
