// kamd_inflate.h -- inflate of one BGZF member (a raw DEFLATE stream, RFC 1951, of at most 64 KiB of text), its CRC-32, and the line
// arithmetic of a FASTQ text: what the kernels of kamd_inflate.hip and the CPU build of tests/emu_inflate share.  Host/device logic, no HIP
// runtime calls.
//
// The decoder is written for `nlanes` cooperating lanes that run it in lockstep (a wavefront: nlanes = 64, `sync` a barrier; the CPU build:
// nlanes = 1, `sync` nothing).  Everything that reads the compressed bits is done by all lanes redundantly -- the bit reader, the block
// headers, the symbols -- so its state is uniform and every lane stores the same values to the shared work area.  The lanes divide
//   * the look-up tables of a block's two codes (entry i = what the canonical decoder finds in the bits of i),
//   * the bytes of a stored block,
//   * the symbols of a round: up to QN symbols are decoded into a queue, then every lane resolves its share of them (a literal is one
//     byte; a match whose source lies wholly in front of the round is copied by one lane), and the matches that read what the round itself
//     produces are copied in stream order, each by all lanes, a match with distance < length as a periodic copy of its first `distance`
//     bytes.  (The match one lane copies alone is a byte loop of that lane, at most 258 steps, periodic too; the other lanes have
//     symbols of their own.  A dependent chain from byte to byte exists nowhere.)
//   * the CRC-32: a slice per lane, the slices' remainders combined by multiplication with x^(8 * bytes behind the slice) mod P.
//
// The redundant part is correct because the lanes are ONE wavefront: they execute every instruction together, so a read-modify-write of
// the work area by all lanes (canon_build's counters and offsets, the code lengths that dynamic_codes writes over the code-length code's)
// reads the same old value and stores the same new one in every lane.  More than one wavefront per member would make these races:
// LANES is the only value of nlanes a device caller may use, and the kernel asserts its block size against it.
//
// Nothing here can run away on bad input: every symbol consumes at least one bit and the consumed bits are compared with the member's
// length after each symbol, every symbol but the end of a block produces at least one byte and the produced bytes are compared with ISIZE
// before they are written.  A stream that breaks a rule is refused with one of the reasons below and decoding stops; there are no asserts.
//
// Which codes are accepted is zlib's rule (inflate_table): over-subscribed codes never; an incomplete code only when its longest code has
// one bit (a single distance code of one bit is what deflate writes for a block with one distance), judged as kamd_pargzip.h judges it; the
// code-length code must be complete.
#pragma once
#include <stdint.h>

#include "kamd_core.h"

namespace kamd {
namespace inf {

enum Reason : int32_t {
  INF_OK = 0,
  INF_SRC_OVERRUN = 1,    // the stream reads beyond its src_len bytes
  INF_DST_OVERRUN = 2,    // ... writes beyond ISIZE
  INF_SHORT = 3,          // ... ends with fewer than ISIZE bytes
  INF_FAR_DISTANCE = 4,   // a distance before the start of the member's output
  INF_BLOCK_TYPE = 5,     // block type 3
  INF_STORED_LEN = 6,     // stored block: LEN != ~NLEN
  INF_BAD_CODE = 7,       // an over-subscribed code, or an incomplete one that zlib does not accept
  INF_BAD_SYMBOL = 8,     // a length / distance symbol outside the defined range, or bits that are no code of the block
  INF_BAD_HEADER = 9,     // dynamic header: more than 286 / 30 codes, a repeat without a previous length or beyond the lengths, no end-of-block code
  INF_CRC = 10            // the text is not what the trailer's CRC-32 says
};

constexpr int QN = 64;          // symbols of a round
constexpr int LIT_TB = 10;      // bits of the literal/length look-up table
constexpr int DIST_TB = 8;      // ... of the distance table
constexpr int LANES = 64;       // the lanes of a wavefront: what `nlanes` is on the device (see above)
constexpr uint32_t MAX_ISIZE = 65536;   // a BGZF member holds at most 64 KiB of text
constexpr uint32_t MAX_SRC_LEN = 1u << 20;   // ... and its stream at most this many bytes (BGZF: 64 KiB with header and trailer): the bit reader's
                                             // 32-bit byte position and the bound "every loop ends with the member's bits" rest on it
constexpr uint32_t CRC_POLY = 0xEDB88320u;

// a canonical Huffman code: how many codes of each length, and the symbols ordered by (length, symbol)
struct Canon { uint16_t count[16]; uint16_t offs[16]; uint16_t sym[288]; };

// the work area of one member (LDS of the wavefront that decodes it)
struct Work {
  uint8_t lens[320];                   // code lengths of the block: literal/length alphabet, then the distances
  Canon cl, lit, dist;
  uint16_t lit_tab[1 << LIT_TB];       // symbol | code length << 9; 0 = the code is longer than the table's bits (or no code at all)
  uint16_t dist_tab[1 << DIST_TB];
  uint32_t crc_tab[256];
  uint16_t q_pos[QN], q_len[QN], q_val[QN];   // symbols a lane resolves alone: len 0 = literal q_val, else a match of distance q_val
  uint16_t d_pos[QN], d_len[QN], d_dist[QN];  // matches that read what this round produces, in stream order
  int32_t has_dist;
};

// ---- bit reader: LSB first, 64-bit buffer, 32 bits at a time; zero bits are invented behind the end and `consumed` tells -------------
struct Bits { const uint8_t* p; uint32_t n; uint32_t pos; uint64_t buf; int32_t cnt; };

// bytes [pos, pos + 4) of the member, zero beyond n.  On the device two aligned dwords (each holds at least one byte of the member, so
// neither leaves the aligned dwords that hold the member's own bytes) instead of four byte loads; the member starts at any address.  The
// first dword may begin up to 3 bytes in front of the member and the last end up to 3 bytes behind it: kamd_bgzf_inflate asks for a
// 4-byte aligned base pointer, so both lie inside the dwords of the caller's own buffer.
KAMD_HD uint32_t src_le32(const uint8_t* p, uint32_t n, uint32_t pos) {
  if (pos >= n) return 0;
  const uint32_t left = n - pos;
#if defined(__HIP_DEVICE_COMPILE__)
  const uintptr_t a = (uintptr_t)(p + pos);
  const uint32_t mis = (uint32_t)(a & 3);
  const uint32_t* w = (const uint32_t*)(a - mis);
  uint32_t v = w[0] >> (8 * mis);
  if (mis && 4 - mis < left) v |= w[1] << (32 - 8 * mis);
#else
  uint32_t v = 0;
  for (uint32_t i = 0; i < 4 && i < left; i++) v |= (uint32_t)p[pos + i] << (8 * i);
#endif
  if (left < 4) v &= (1u << (8 * left)) - 1;
  return v;
}
KAMD_HD void bits_seek(Bits& b, uint32_t byte) { b.pos = byte; b.buf = 0; b.cnt = 0; }
KAMD_HD void bits_refill(Bits& b) {   // at least 33 bits afterwards
  while (b.cnt <= 32) { b.buf |= (uint64_t)src_le32(b.p, b.n, b.pos) << b.cnt; b.pos += 4; b.cnt += 32; }
}
KAMD_HD uint64_t bits_consumed(const Bits& b) { return (uint64_t)b.pos * 8 - (uint64_t)b.cnt; }
KAMD_HD bool bits_overrun(const Bits& b) { return bits_consumed(b) > (uint64_t)b.n * 8; }
KAMD_HD uint32_t bits_take(Bits& b, int k) { const uint32_t v = (uint32_t)(b.buf & ((1ull << k) - 1)); b.buf >>= k; b.cnt -= k; return v; }

// ---- canonical codes -------------------------------------------------------------------------------------------------------------
// kind 0: literal/length, 1: distance, 2: code-length code.  Serial (every lane does the same).
KAMD_HD int canon_build(const uint8_t* lens, int n, int kind, Canon* c) {
  for (int l = 0; l < 16; l++) c->count[l] = 0;
  for (int i = 0; i < n; i++) c->count[lens[i] & 15]++;
  c->count[0] = 0;
  int left = 1, maxlen = 0, used = 0;
  for (int l = 1; l <= 15; l++) {
    left <<= 1; left -= c->count[l];
    if (left < 0) return INF_BAD_CODE;
    if (c->count[l]) maxlen = l;
    used += c->count[l];
  }
  if (left > 0 && (kind == 2 || maxlen > 1)) return INF_BAD_CODE;   // incomplete: only a code of one-bit codes may be (zlib's inflate_table)
  if (kind != 1 && used == 0) return INF_BAD_CODE;
  uint16_t o = 0;
  for (int l = 1; l <= 15; l++) { c->offs[l] = o; o = (uint16_t)(o + c->count[l]); }
  for (int i = 0; i < n; i++) { const int l = lens[i] & 15; if (l) c->sym[c->offs[l]++] = (uint16_t)i; }
  return INF_OK;
}
// the symbol whose code the low bits of `bits` start with (first bit of the stream = bit 0), looking at `maxbits` of them; -1: none
KAMD_HD int canon_decode(const Canon& c, uint32_t bits, int maxbits, int* len) {
  int code = 0, first = 0, index = 0;
  for (int l = 1; l <= maxbits; l++) {
    code |= (int)(bits & 1); bits >>= 1;
    const int cnt = c.count[l];
    if (code - cnt < first) { *len = l; return c.sym[index + (code - first)]; }
    index += cnt; first += cnt; first <<= 1; code <<= 1;
  }
  return -1;
}
KAMD_HD void fill_table(const Canon& c, uint16_t* tab, int tb, int lane, int nlanes) {
  for (int i = lane; i < (1 << tb); i += nlanes) {
    int l = 0;
    const int s = canon_decode(c, (uint32_t)i, tb, &l);
    tab[i] = s < 0 ? (uint16_t)0 : (uint16_t)(s | (l << 9));
  }
}
KAMD_HD int table_decode(const Canon& c, const uint16_t* tab, int tb, Bits& b) {   // -1: the bits are no code
  const uint32_t e = tab[b.buf & ((1u << tb) - 1)];
  int l = (int)(e >> 9), s = (int)(e & 511);
  if (!l) { s = canon_decode(c, (uint32_t)b.buf, 15, &l); if (s < 0) return -1; }
  b.buf >>= l; b.cnt -= l;
  return s;
}

KAMD_HD int cl_order(int i) {   // the order in which a dynamic header stores the lengths of the code-length code
#define KAMD_P5(v, j) ((uint64_t)(v) << (5 * (j)))
  const uint64_t lo = KAMD_P5(16, 0) | KAMD_P5(17, 1) | KAMD_P5(18, 2) | KAMD_P5(0, 3) | KAMD_P5(8, 4) | KAMD_P5(7, 5) | KAMD_P5(9, 6) | KAMD_P5(6, 7) |
                      KAMD_P5(10, 8) | KAMD_P5(5, 9) | KAMD_P5(11, 10) | KAMD_P5(4, 11);
  const uint64_t hi = KAMD_P5(12, 0) | KAMD_P5(3, 1) | KAMD_P5(13, 2) | KAMD_P5(2, 3) | KAMD_P5(14, 4) | KAMD_P5(1, 5) | KAMD_P5(15, 6);
#undef KAMD_P5
  return (int)((i < 12 ? lo >> (5 * i) : hi >> (5 * (i - 12))) & 31);
}

// the codes of a fixed block / of the dynamic header behind BTYPE; serial.  Leaves w.lit, w.dist, w.has_dist (the tables: fill_table)
KAMD_HD int fixed_codes(Work& w) {
  for (int i = 0; i < 288; i++) w.lens[i] = (uint8_t)(i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : 8);
  for (int i = 0; i < 32; i++) w.lens[288 + i] = 5;
  w.has_dist = 1;
  if (int r = canon_build(w.lens, 288, 0, &w.lit)) return r;
  return canon_build(w.lens + 288, 32, 1, &w.dist);
}
KAMD_HD int dynamic_codes(Bits& b, Work& w) {
  bits_refill(b);
  const int hlit = (int)bits_take(b, 5) + 257, hdist = (int)bits_take(b, 5) + 1, hclen = (int)bits_take(b, 4) + 4;
  if (hlit > 286 || hdist > 30) return INF_BAD_HEADER;
  for (int i = 0; i < 19; i++) w.lens[i] = 0;
  for (int i = 0; i < hclen; i++) { bits_refill(b); w.lens[cl_order(i)] = (uint8_t)bits_take(b, 3); }
  if (int r = canon_build(w.lens, 19, 2, &w.cl)) return r;
  const int total = hlit + hdist;   // (w.cl no longer needs w.lens: the block's lengths take its place)
  uint8_t* lens = w.lens;
  int i = 0;
  while (i < total) {
    bits_refill(b);
    int l = 0;
    const int sym = canon_decode(w.cl, (uint32_t)b.buf, 7, &l);
    if (sym < 0) return INF_BAD_SYMBOL;
    b.buf >>= l; b.cnt -= l;
    if (sym < 16) lens[i++] = (uint8_t)sym;
    else {
      int rep; uint8_t v = 0;
      if (sym == 16) { if (i == 0) return INF_BAD_HEADER; v = lens[i - 1]; rep = 3 + (int)bits_take(b, 2); }
      else if (sym == 17) rep = 3 + (int)bits_take(b, 3);
      else rep = 11 + (int)bits_take(b, 7);
      if (i + rep > total) return INF_BAD_HEADER;   // (a run may cross from the literal/length lengths into the distances, not beyond them)
      while (rep--) lens[i++] = v;
    }
    if (bits_overrun(b)) return INF_SRC_OVERRUN;
  }
  if (lens[256] == 0) return INF_BAD_HEADER;   // no end-of-block code
  if (int r = canon_build(lens, hlit, 0, &w.lit)) return r;
  int any = 0;
  for (int j = 0; j < hdist; j++) any |= lens[hlit + j];
  w.has_dist = any != 0;   // no distance code at all is a valid block of literals; a length symbol in it is refused
  if (any) if (int r = canon_build(lens + hlit, hdist, 1, &w.dist)) return r;
  return INF_OK;
}

// ---- a round: up to QN symbols into the queues; serial and uniform ---------------------------------------------------------------
// *opos advances behind what the queued symbols produce; *eob: the block's end code was met
KAMD_HD int decode_round(Bits& b, Work& w, uint32_t isize, uint32_t* opos, int* nq, int* nd, bool* eob) {
  const uint32_t round_start = *opos;
  uint32_t o = round_start;
  int q = 0, d = 0;
  *eob = false;
  while (q < QN && d < QN) {
    bits_refill(b);
    const int s = table_decode(w.lit, w.lit_tab, LIT_TB, b);
    if (s < 0) return INF_BAD_SYMBOL;
    if (s < 256) {
      if (o >= isize) return INF_DST_OVERRUN;
      w.q_pos[q] = (uint16_t)o; w.q_len[q] = 0; w.q_val[q] = (uint16_t)s; ++q; ++o;
    } else if (s == 256) {
      *eob = true;
      if (bits_overrun(b)) return INF_SRC_OVERRUN;
      break;
    } else {
      if (s > 285 || !w.has_dist) return INF_BAD_SYMBOL;
      const int li = s - 257;
      uint32_t len;
      if (li < 8) len = 3u + (uint32_t)li;
      else if (li == 28) len = 258;
      else { const int e = (li >> 2) - 1; len = 3u + ((4u + (uint32_t)(li & 3)) << e) + bits_take(b, e); }
      bits_refill(b);
      const int ds = table_decode(w.dist, w.dist_tab, DIST_TB, b);
      if (ds < 0 || ds > 29) return INF_BAD_SYMBOL;
      uint32_t dist;
      if (ds < 4) dist = 1u + (uint32_t)ds;
      else { const int e = (ds >> 1) - 1; dist = 1u + ((2u + (uint32_t)(ds & 1)) << e) + bits_take(b, e); }
      if (dist > o) return INF_FAR_DISTANCE;
      if (len > isize - o) return INF_DST_OVERRUN;
      const uint32_t src_end = o - dist + (len < dist ? len : dist);   // the bytes the copy reads lie in front of this
      if (src_end <= round_start) { w.q_pos[q] = (uint16_t)o; w.q_len[q] = (uint16_t)len; w.q_val[q] = (uint16_t)(dist - 1); ++q; }
      else { w.d_pos[d] = (uint16_t)o; w.d_len[d] = (uint16_t)len; w.d_dist[d] = (uint16_t)(dist - 1); ++d; }
      o += len;
    }
    if (bits_overrun(b)) return INF_SRC_OVERRUN;
  }
  *opos = o; *nq = q; *nd = d;
  return INF_OK;
}
// what the lanes do with a decoded round.  `out` is the member's text from its first byte (the whole member stays in LDS, so a back-reference
// never reads global memory).  (Distances are queued minus one: 32 768 does not fit 16 bits next to 0.)
template <class Sync>
KAMD_HD void resolve_round(Work& w, uint8_t* out, int nq, int nd, int lane, int nlanes, Sync&& sync) {
  sync();   // the queues are written
  for (int i = lane; i < nq; i += nlanes) {
    const uint32_t pos = w.q_pos[i], len = w.q_len[i];
    if (!len) { out[pos] = (uint8_t)w.q_val[i]; continue; }
    const uint32_t dist = (uint32_t)w.q_val[i] + 1;
    const uint8_t* src = out + pos - dist;
    for (uint32_t j = 0, s = 0; j < len; j++) { out[pos + j] = src[s]; if (++s == dist) s = 0; }
  }
  sync();
  for (int k = 0; k < nd; k++) {
    const uint32_t pos = w.d_pos[k], len = w.d_len[k], dist = (uint32_t)w.d_dist[k] + 1;
    const uint8_t* src = out + pos - dist;   // [pos - dist, pos) is final: everything in front of this match has been written
    for (uint32_t j = (uint32_t)lane; j < len; j += (uint32_t)nlanes) out[pos + j] = src[dist < len ? j % dist : j];
    sync();
  }
}

// ---- the member ----------------------------------------------------------------------------------------------------------------------
// Decodes src[0, n) into out[0, isize).  Every lane returns the same reason.
template <class Sync>
KAMD_HD int inflate_member(const uint8_t* src, uint32_t n, uint8_t* out, uint32_t isize, Work& w, int lane, int nlanes, Sync&& sync) {
  Bits b{src, n, 0, 0, 0};
  uint32_t opos = 0;
  for (;;) {   // a block consumes at least three bits, and the consumed bits are checked below: at most 8 n / 3 blocks
    bits_refill(b);
    const uint32_t bfinal = bits_take(b, 1), btype = bits_take(b, 2);
    if (bits_overrun(b)) return INF_SRC_OVERRUN;
    if (btype == 3) return INF_BLOCK_TYPE;
    if (btype == 0) {
      bits_take(b, b.cnt & 7);   // to the byte boundary (cnt and the consumed bits are congruent mod 8)
      bits_refill(b);
      const uint32_t len = bits_take(b, 16), nlen = bits_take(b, 16);
      if (bits_overrun(b)) return INF_SRC_OVERRUN;
      if ((len ^ nlen) != 0xFFFFu) return INF_STORED_LEN;
      const uint32_t at = (uint32_t)(bits_consumed(b) >> 3);
      if (len > n - at) return INF_SRC_OVERRUN;
      if (len > isize - opos) return INF_DST_OVERRUN;
      for (uint32_t j = 4u * (uint32_t)lane; j < len; j += 4u * (uint32_t)nlanes) {
        const uint32_t v = src_le32(src, n, at + j);
        for (uint32_t i = 0; i < 4 && j + i < len; i++) out[opos + j + i] = (uint8_t)(v >> (8 * i));
      }
      opos += len;
      bits_seek(b, at + len);
      sync();
    } else {
      sync();   // (nobody still reads the previous block's tables)
      const int r = btype == 1 ? fixed_codes(w) : dynamic_codes(b, w);
      if (r) return r;
      sync();
      fill_table(w.lit, w.lit_tab, LIT_TB, lane, nlanes);
      if (w.has_dist) fill_table(w.dist, w.dist_tab, DIST_TB, lane, nlanes);
      sync();
      for (;;) {   // a round that is not the block's last produces at least QN bytes
        int nq = 0, nd = 0; bool eob = false;
        const int rr = decode_round(b, w, isize, &opos, &nq, &nd, &eob);
        if (rr) return rr;
        resolve_round(w, out, nq, nd, lane, nlanes, sync);
        if (eob) break;
      }
    }
    if (bfinal) break;
  }
  return opos == isize ? INF_OK : INF_SHORT;
}

// ---- CRC-32 (the gzip polynomial, reflected) ----------------------------------------------------------------------------------------
KAMD_HD void crc_table_fill(uint32_t* tab, int lane, int nlanes) {
  for (int i = lane; i < 256; i += nlanes) {
    uint32_t c = (uint32_t)i;
    for (int k = 0; k < 8; k++) c = (c >> 1) ^ ((c & 1) ? CRC_POLY : 0u);
    tab[i] = c;
  }
}
// a * b mod P; bit 31 is the coefficient of x^0
KAMD_HD uint32_t gf_mul(uint32_t a, uint32_t b) {
  uint32_t p = 0;
  for (int i = 0; i < 32; i++) { if (a & 0x80000000u) p ^= b; a <<= 1; b = (b >> 1) ^ ((b & 1) ? CRC_POLY : 0u); }
  return p;
}
KAMD_HD uint32_t gf_xpow(uint64_t n) {   // x^n mod P
  uint32_t p = 0x80000000u, base = 0x40000000u;
  for (; n; n >>= 1) { if (n & 1) p = gf_mul(p, base); base = gf_mul(base, base); }
  return p;
}
// Lane `lane` of `nlanes` takes bytes [lane * S, (lane + 1) * S) of buf[0, n), S = ceil(n / nlanes): the register after its bytes (lane 0
// starts from all ones, the others from zero) times x^(8 * bytes behind the slice).  The XOR of all lanes' terms, inverted, is the CRC-32.
// *newlines: the '\n' of the slice.
KAMD_HD uint32_t crc_slice_term(const uint8_t* buf, uint32_t n, const uint32_t* tab, int lane, int nlanes, uint32_t* newlines) {
  const uint32_t S = (n + (uint32_t)nlanes - 1) / (uint32_t)nlanes;
  const uint64_t lo64 = (uint64_t)lane * S;
  const uint32_t lo = lo64 < n ? (uint32_t)lo64 : n, hi = n - lo < S ? n : lo + S;
  uint32_t c = lane == 0 ? 0xFFFFFFFFu : 0u, nl = 0;
  for (uint32_t i = lo; i < hi; i++) { const uint8_t x = buf[i]; nl += x == '\n'; c = tab[(c ^ x) & 0xFF] ^ (c >> 8); }
  *newlines = nl;
  if (lane != 0 && lo == hi) return 0;
  return gf_mul(c, gf_xpow(8ull * (n - hi)));
}

// ---- lines of a text ----------------------------------------------------------------------------------------------------------------
constexpr uint64_t TEXT_CHUNK = 16384;   // partial newline counts are kept per chunk of the text (a quarter of a member)

KAMD_HD uint32_t nl_count32(uint32_t w) {   // bytes of w that are '\n' (exact: no carries between bytes)
  const uint32_t x = w ^ 0x0A0A0A0Au;
  const uint32_t nz = ((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x;   // bit 7 of every byte that is not zero
  return (uint32_t)__builtin_popcount(~nz & 0x80808080u);
}
// '\n' in t[lo, hi): bytes up to an aligned address, aligned 8-byte words, bytes
KAMD_HD uint64_t lines_range(const uint8_t* t, uint64_t lo, uint64_t hi) {
  uint64_t c = 0, i = lo;
  for (; i < hi && ((uintptr_t)(t + i) & 7); i++) c += t[i] == '\n';
  for (; i + 8 <= hi; i += 8) { uint64_t w; __builtin_memcpy(&w, t + i, 8); c += nl_count32((uint32_t)w) + nl_count32((uint32_t)(w >> 32)); }
  for (; i < hi; i++) c += t[i] == '\n';
  return c;
}
// the offset just behind newline number r (1-based) of t[lo, hi); hi when there are fewer
KAMD_HD uint64_t locate_in(const uint8_t* t, uint64_t lo, uint64_t hi, uint64_t r) {
  for (uint64_t i = lo; i < hi; i++) if (t[i] == '\n' && --r == 0) return i + 1;
  return hi;
}
// the chunk that holds newline number k (1-based) of the text, from the chunks' counts; *r = its number inside that chunk.  n_chunks: none
KAMD_HD uint64_t locate_chunk(const uint32_t* counts, uint64_t n_chunks, uint64_t k, uint64_t* r) {
  uint64_t before = 0;
  for (uint64_t c = 0; c < n_chunks; c++) { if (before + counts[c] >= k) { *r = k - before; return c; } before += counts[c]; }
  *r = 0;
  return n_chunks;
}
// whole records at the head of the texts: records = min over the files of lines / 4, at most max_records
KAMD_HD uint64_t records_of(const uint64_t* lines, int n_files, uint64_t max_records) {
  uint64_t r = max_records;
  for (int f = 0; f < n_files; f++) if (lines[f] / 4 < r) r = lines[f] / 4;
  return r;
}

}  // namespace inf
}  // namespace kamd
