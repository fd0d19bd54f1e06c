// BGZF / DEFLATE decoder core: RFC 1951 (deflate), RFC 1952 (the gzip member around it) and the BGZF section of the SAM
// specification (a gzip member of at most 64 KiB with its own size in a `BC` extra subfield).  Replaces the inflate of
// `zcat F.fastq.gz | ...` (runRufus.sh:157-160).
//
// Written ONCE, for host and device: every function is RFX_BGZF_HD (`__host__ __device__` under hipcc, `inline` under a
// host compiler), so the statements the kernel runs (rfx_bgzf.hip) are the statements tests/host/bgzf_harness.cpp runs
// under AddressSanitizer and UBSan on the CPU.  What differs is only WHERE the decoded bytes go: bgzf_inflate takes an
// output policy `Out` with
//     void literal(uint32_t pos, uint32_t byte);                    // out[pos] = byte
//     void match(uint32_t pos, uint32_t len, uint32_t dist);        // out[pos + i] = out[pos - dist + i % dist], i < len
//     void stored(uint32_t pos, const uint8_t* src, uint32_t n);    // out[pos + i] = src[i], i < n
//     void end();
// The host policy is a serial copy; the kernel's spreads a literal run, a match or a stored run over the 64 lanes.
//
// Bounds.  The core reads input only through bgzf_bits, which never touches a byte outside [p, end), and hands `stored`
// a source range it has checked to lie inside [p, end).  It writes only to the table arrays of the bgzf_tables it is
// given, at indices bounded by the arrays' sizes (a symbol is < 320, a code length < 16, a peeked index < the fast
// table's size).  It calls the policy only with pos + len <= isize and, for a match, dist <= pos: a block is independent
// (no history from the block before), so nothing outside [out, out + isize) of a block is ever read or written,
// whatever the input says.
//
// On the device the whole wave runs these statements with uniform control flow: all 64 lanes compute the same values and
// store them to the same table words, read-modify-writes (`count[l]++`, `symbol[offs[l]++]`) included.  That is right
// only because a wave64 executes in lockstep -- the kernel's workgroup is ONE wave (`__launch_bounds__(64)`) and nothing
// in here depends on the lane -- so every lane reads the old word before any lane's store of the new one lands.  (The
// table clears and builds are therefore serial; the lanes could share them.)
//
// Termination.  Every loop in this file either runs a number of times fixed by a table size (<= 1024 iterations: the
// table builds, the CRC's 8 / 32 steps), or consumes at least one input bit, or emits at least one output byte, or
// returns an error: bgzf_decode consumes the bits of the code it returns (a code is >= 1 bit long) or fails; a block
// header is 3 bits; a code-length symbol is >= 1 bit; a literal or a match emits bytes.  A block therefore ends after at
// most 8 * (end - p) + isize steps.
#pragma once
#include <stdint.h>

#if defined(__HIP__)  // (compiled as HIP: the kernel's translation unit)
#include <hip/hip_runtime.h>
#define RFX_BGZF_HD __host__ __device__ __forceinline__
#else
#define RFX_BGZF_HD inline
#endif
// Statistics hook of the host harness (coverage of the decoder's branches); nothing in the library or the kernel.
#ifndef RFX_BGZF_STAT
#define RFX_BGZF_STAT(x) ((void)0)
#endif

enum bgzf_status : uint32_t {
  BGZF_OK = 0,
  BGZF_E_BTYPE = 1,        // block type 3
  BGZF_E_STORED_LEN = 2,   // stored block: LEN != ~NLEN
  BGZF_E_HLIT_HDIST = 3,   // HLIT > 286 or HDIST > 30
  BGZF_E_OVERSUB = 4,      // over-subscribed code lengths
  BGZF_E_INCOMPLETE = 5,   // incomplete code lengths (other than RFC 1951's single code of one bit)
  BGZF_E_REP_NOPREV = 6,   // repeat code 16 with no previous length
  BGZF_E_CL_RUN = 7,       // a code-length run past HLIT + HDIST
  BGZF_E_NO_EOB = 8,       // no end-of-block code
  BGZF_E_LITLEN_SYM = 9,   // literal/length symbol 286 / 287
  BGZF_E_DIST_SYM = 10,    // distance symbol 30 / 31
  BGZF_E_DIST_FAR = 11,    // a distance reaching before the block's first output byte
  BGZF_E_OUT_OVER = 12,    // output beyond ISIZE
  BGZF_E_OUT_SHORT = 13,   // output short of ISIZE at the final block
  BGZF_E_IN_END = 14,      // input exhausted
  BGZF_E_TRAILING = 15,    // the deflate stream does not end in the payload's last byte
  BGZF_E_CRC = 16,         // CRC-32 mismatch
  BGZF_E_CODE = 17,        // bits that are no code of an incomplete (single-code or empty) table
  BGZF_STATUS_COUNT = 18
};

inline const char* bgzf_status_text(uint32_t s) {
  static const char* const text[BGZF_STATUS_COUNT] = {
      "ok", "block type 3", "stored block: LEN is not ~NLEN", "HLIT > 286 or HDIST > 30", "over-subscribed code lengths",
      "incomplete code lengths", "repeat code 16 with no previous length", "code-length run past HLIT + HDIST",
      "no end-of-block code", "literal/length symbol 286 or 287", "distance symbol 30 or 31",
      "distance reaches before the block's first byte", "output beyond ISIZE", "output short of ISIZE", "input exhausted",
      "deflate stream does not end in the payload's last byte", "CRC mismatch", "bits that are no code"};
  return s < BGZF_STATUS_COUNT ? text[s] : "unknown status";
}

// What the kernel is told about one BGZF block (built on the host from the scan).
struct bgzf_desc {
  uint64_t in_off;   // deflate payload: byte offset in the staging buffer
  uint64_t out_off;  // where the block's bytes go: byte offset in the arena
  uint32_t in_len;   // payload bytes
  uint32_t isize;    // inflated bytes (<= 65536)
  uint32_t crc;      // CRC-32 of the inflated bytes (the footer's)
  uint32_t pad;
};

// ---- BGZF block header (host side: rfx_bgzf_scan, the harness) -------------------------------------------------------
// 0: a whole block lies in [b, b + avail): *bsize = its size, *pay_off / *pay_len = its deflate payload, *isize, *crc;
// 1: what is there is a valid beginning of a block, but not a whole one;  -1: not BGZF.
inline int bgzf_block_header(const uint8_t* b, uint64_t avail, uint32_t* bsize, uint32_t* pay_off, uint32_t* pay_len,
                             uint32_t* isize, uint32_t* crc) {
  static const uint8_t magic[3] = {0x1f, 0x8b, 0x08};
  for (uint64_t i = 0; i < 3 && i < avail; ++i)
    if (b[i] != magic[i]) return -1;
  if (avail > 3 && b[3] != 4) return -1;  // FLG: FEXTRA and nothing else (BGZF; a name or comment field would sit before the payload)
  if (avail < 12) return 1;
  const uint32_t xlen = b[10] | (uint32_t)b[11] << 8;
  if (avail < 12ull + xlen) return 1;
  uint32_t bs = 0, at = 0;
  bool found = false;
  while (at + 4 <= xlen) {  // SI1 SI2 SLEN(2) data: the BC subfield need not be the first
    const uint8_t* f = b + 12 + at;
    const uint32_t slen = f[2] | (uint32_t)f[3] << 8;
    if (at + 4 + slen > xlen) return -1;
    if (f[0] == 'B' && f[1] == 'C' && slen == 2 && !found) {
      bs = (f[4] | (uint32_t)f[5] << 8) + 1u;
      found = true;
    }
    at += 4 + slen;
  }
  if (!found || at != xlen || bs < 12 + xlen + 8) return -1;
  if (avail < bs) return 1;
  const uint8_t* ft = b + bs - 8;
  const uint32_t is = ft[4] | (uint32_t)ft[5] << 8 | (uint32_t)ft[6] << 16 | (uint32_t)ft[7] << 24;
  if (is > 65536u) return -1;
  *bsize = bs;
  *pay_off = 12 + xlen;
  *pay_len = bs - 12 - xlen - 8;
  *isize = is;
  *crc = ft[0] | (uint32_t)ft[1] << 8 | (uint32_t)ft[2] << 16 | (uint32_t)ft[3] << 24;
  return 0;
}

// ---- bit reader over [p, end) -------------------------------------------------------------------------------------------
// `bits` holds n valid bits (the next bit of the stream is bit 0).  Bits above n are either zero or already the stream's
// next bits (the 8-byte refill reads ahead of what it counts), so OR-ing the same bytes in again changes nothing.
struct bgzf_bits {
  const uint8_t* p;
  const uint8_t* end;
  uint64_t bits;
  uint32_t n;
};
RFX_BGZF_HD void bgzf_bits_init(bgzf_bits& b, const uint8_t* p, const uint8_t* end) {
  b.p = p;
  b.end = end;
  b.bits = 0;
  b.n = 0;
}
RFX_BGZF_HD void bgzf_refill(bgzf_bits& b) {  // afterwards n >= 56, or every byte of the input is in
  if (b.end - b.p >= 8) {
    const uint8_t* q = b.p;
    const uint64_t w = (uint64_t)q[0] | (uint64_t)q[1] << 8 | (uint64_t)q[2] << 16 | (uint64_t)q[3] << 24 | (uint64_t)q[4] << 32 |
                       (uint64_t)q[5] << 40 | (uint64_t)q[6] << 48 | (uint64_t)q[7] << 56;
    b.bits |= w << b.n;  // (n <= 63; a wave-uniform amount in the kernel)
    const uint32_t took = (63u - b.n) >> 3;
    b.p += took;
    b.n += took * 8u;
  } else {
    while (b.n <= 56u && b.p < b.end) {
      b.bits |= (uint64_t)*b.p++ << b.n;
      b.n += 8u;
    }
  }
}
RFX_BGZF_HD uint32_t bgzf_peek(const bgzf_bits& b, uint32_t k) { return (uint32_t)b.bits & ((1u << k) - 1u); }  // k <= 16
RFX_BGZF_HD void bgzf_drop(bgzf_bits& b, uint32_t k) {  // k <= n, k < 64
  b.bits >>= k;
  b.n -= k;
}

// ---- Huffman tables ---------------------------------------------------------------------------------------------------
// Canonical code as count-per-length + symbols in code order (decodes any code bit by bit), and in front of it a table
// over the next `fast_bits` bits for the codes that short: entry = length << 9 | symbol, 0 = longer code (or none).
struct bgzf_huff {
  uint16_t* count;   // [16]
  uint16_t* offs;    // [16] scratch of the build
  uint16_t* symbol;  // [n symbols]
  uint16_t* fast;    // [1 << fast_bits]
  uint32_t fast_bits;
};
constexpr uint32_t BGZF_LIT_FAST = 10, BGZF_DIST_FAST = 9, BGZF_CLC_FAST = 7;
constexpr uint32_t BGZF_MAX_LIT = 288, BGZF_MAX_DIST = 32;
// One decoder's tables: 4160 bytes.  (The code-length code borrows the distance code's arrays: it is done with before the
// distance code is built.)
struct bgzf_tables {
  uint16_t lit_fast[1u << BGZF_LIT_FAST];
  uint16_t dist_fast[1u << BGZF_DIST_FAST];
  uint16_t lit_symbol[BGZF_MAX_LIT];
  uint16_t dist_symbol[BGZF_MAX_DIST];
  uint16_t lit_count[16], lit_offs[16], dist_count[16], dist_offs[16];
  uint8_t lengths[BGZF_MAX_LIT + BGZF_MAX_DIST];
};
RFX_BGZF_HD bgzf_huff bgzf_lit_huff(bgzf_tables& t) { return bgzf_huff{t.lit_count, t.lit_offs, t.lit_symbol, t.lit_fast, BGZF_LIT_FAST}; }
RFX_BGZF_HD bgzf_huff bgzf_dist_huff(bgzf_tables& t) { return bgzf_huff{t.dist_count, t.dist_offs, t.dist_symbol, t.dist_fast, BGZF_DIST_FAST}; }
RFX_BGZF_HD bgzf_huff bgzf_clc_huff(bgzf_tables& t) { return bgzf_huff{t.dist_count, t.dist_offs, t.dist_symbol, t.dist_fast, BGZF_CLC_FAST}; }

RFX_BGZF_HD uint32_t bgzf_rev(uint32_t code, uint32_t len) {  // the low `len` bits, reversed (len <= 15)
  uint32_t r = 0;
  for (uint32_t i = 0; i < 15u; ++i)
    if (i < len) r |= ((code >> i) & 1u) << (len - 1u - i);
  return r;
}

// Builds h from lengths[0 .. n) (n <= the symbol array's size, every length <= 15).  BGZF_OK for a complete code, for the
// single code of one bit where allow_single says so (the literal/length and the distance code, as zlib accepts them; never
// the code-length code), and -- allow_empty -- for no code at all (a block of literals only has no distance code);
// *max_len = the longest code.
RFX_BGZF_HD uint32_t bgzf_build(bgzf_huff& h, const uint8_t* lengths, uint32_t n, bool allow_empty, bool allow_single,
                                uint32_t* max_len) {
  for (uint32_t l = 0; l < 16u; ++l) h.count[l] = 0;
  for (uint32_t s = 0; s < n; ++s) h.count[lengths[s] & 15u]++;
  const uint32_t size = 1u << h.fast_bits;
  for (uint32_t i = 0; i < size; ++i) h.fast[i] = 0;
  uint32_t mx = 0;
  int32_t left = 1;
  for (uint32_t l = 1; l < 16u; ++l) {
    left = left * 2 - (int32_t)h.count[l];
    if (left < 0) return BGZF_E_OVERSUB;
    if (h.count[l]) mx = l;
  }
  *max_len = mx;
  if (mx == 0) return allow_empty ? BGZF_OK : BGZF_E_INCOMPLETE;
  if (left > 0 && !(allow_single && mx == 1 && h.count[1] == 1)) return BGZF_E_INCOMPLETE;
  h.offs[1] = 0;
  for (uint32_t l = 1; l < 15u; ++l) h.offs[l + 1] = (uint16_t)(h.offs[l] + h.count[l]);
  for (uint32_t s = 0; s < n; ++s) {
    const uint32_t l = lengths[s] & 15u;
    if (l) h.symbol[h.offs[l]++] = (uint16_t)s;  // (offs[l] < number of coded symbols <= n)
  }
  uint32_t code = 0, idx = 0;
  for (uint32_t l = 1; l <= h.fast_bits; ++l) {  // the symbols are in code order: the code goes up by one per symbol
    for (uint32_t i = 0; i < h.count[l]; ++i) {
      const uint32_t e = l << 9 | h.symbol[idx++];
      for (uint32_t j = bgzf_rev(code, l); j < size; j += 1u << l) h.fast[j] = (uint16_t)e;
      ++code;
    }
    code <<= 1;
  }
  return BGZF_OK;
}

// The next symbol of h, its bits consumed; >= 0x10000: BGZF_E_* << 16.  Wants >= 15 bits in the buffer (a code is <= 15
// bits) or, with fewer, bgzf_refill to have found the input at its end.
RFX_BGZF_HD uint32_t bgzf_decode(bgzf_bits& b, const bgzf_huff& h) {
  const uint32_t e = h.fast[(uint32_t)b.bits & ((1u << h.fast_bits) - 1u)];
  if (e) {
    const uint32_t l = e >> 9;
    if (l > b.n) return (uint32_t)BGZF_E_IN_END << 16;
    bgzf_drop(b, l);
    return e & 511u;
  }
  uint32_t code = 0, first = 0, index = 0;
  for (uint32_t l = 1; l < 16u; ++l) {
    if (l > b.n) return (uint32_t)BGZF_E_IN_END << 16;
    code |= (uint32_t)(b.bits >> (l - 1u)) & 1u;
    const uint32_t cnt = h.count[l];
    if (code < first + cnt) {
      bgzf_drop(b, l);
      return h.symbol[index + (code - first)];
    }
    index += cnt;
    first = (first + cnt) << 1;
    code <<= 1;
  }
  return (uint32_t)BGZF_E_CODE << 16;
}

// RFC 1951 section 3.2.5's tables in closed form: length symbol 257 .. 285 and distance symbol 0 .. 29 -> base, extra bits
RFX_BGZF_HD uint32_t bgzf_len_base(uint32_t sym, uint32_t* extra) {
  if (sym < 265u) { *extra = 0; return sym - 254u; }
  if (sym == 285u) { *extra = 0; return 258u; }
  const uint32_t e = (sym - 261u) >> 2;
  *extra = e;
  return ((4u + ((sym - 265u) & 3u)) << e) + 3u;
}
RFX_BGZF_HD uint32_t bgzf_dist_base(uint32_t sym, uint32_t* extra) {
  if (sym < 4u) { *extra = 0; return sym + 1u; }
  const uint32_t e = (sym >> 1) - 1u;
  *extra = e;
  return ((2u + (sym & 1u)) << e) + 1u;
}

// ---- CRC-32 (polynomial 0xEDB88320, reflected) ------------------------------------------------------------------------
// The REGISTER is what these work on (no pre- or post-inversion): crc32(data) = ~bgzf_crc_update(0xFFFFFFFF, data).  The
// register is linear in its start value, so for a block cut into slices
//     reg(A || B) = bgzf_crc_shift(reg(A), |B|) ^ bgzf_crc_update(0, B)
// and 64 lanes can each take a slice: the first starts from 0xFFFFFFFF, the others from 0, each shifts its register by
// the bytes behind its slice, and the XOR of all is the block's register.
RFX_BGZF_HD uint32_t bgzf_crc_update(uint32_t reg, const uint8_t* p, uint32_t n) {
  for (uint32_t i = 0; i < n; ++i) {
    reg ^= p[i];
    for (int k = 0; k < 8; ++k) reg = (reg >> 1) ^ (0xEDB88320u & (0u - (reg & 1u)));
  }
  return reg;
}
RFX_BGZF_HD uint32_t bgzf_crc_mul(uint32_t a, uint32_t b) {  // a * b mod P; bit 31 is x^0
  uint32_t p = 0;
  for (uint32_t i = 0; i < 32u; ++i) {
    p ^= b & (0u - ((a >> (31u - i)) & 1u));
    b = (b >> 1) ^ (0xEDB88320u & (0u - (b & 1u)));
  }
  return p;
}
RFX_BGZF_HD uint32_t bgzf_crc_shift(uint32_t reg, uint32_t n_bytes) {  // the register after n_bytes more zero bytes of a zero start
  uint32_t r = 0x80000000u, sq = 0x00800000u;                        // 1, x^8
  for (uint32_t i = 0; i < 32u; ++i) {
    if ((n_bytes >> i) & 1u) r = bgzf_crc_mul(r, sq);
    sq = bgzf_crc_mul(sq, sq);
  }
  return bgzf_crc_mul(reg, r);
}
// The block's CRC-32 the way the kernel computes it, lane by lane (lane = 0 .. 63; XOR the results, then invert).
RFX_BGZF_HD uint32_t bgzf_crc_lane(const uint8_t* out, uint32_t isize, uint32_t lane) {
  const uint32_t slice = (isize + 63u) / 64u;
  const uint32_t lo = lane * slice < isize ? lane * slice : isize;
  const uint32_t hi = lo + slice < isize ? lo + slice : isize;
  const uint32_t reg = bgzf_crc_update(lane == 0 ? 0xFFFFFFFFu : 0u, out + lo, hi - lo);
  return bgzf_crc_shift(reg, isize - hi);
}

// ---- one BGZF block's deflate stream ------------------------------------------------------------------------------------
template <class Out>
RFX_BGZF_HD uint32_t bgzf_inflate(const uint8_t* p, const uint8_t* end, uint32_t isize, bgzf_tables& t, Out& out) {
  bgzf_bits b;
  bgzf_bits_init(b, p, end);
  uint32_t pos = 0;
  for (;;) {  // one deflate block per turn: >= 3 bits
    bgzf_refill(b);
    if (b.n < 3u) return BGZF_E_IN_END;
    const uint32_t final_block = bgzf_peek(b, 1), type = (bgzf_peek(b, 3) >> 1);
    bgzf_drop(b, 3);
    RFX_BGZF_STAT(block(type));
    if (type == 3u) return BGZF_E_BTYPE;
    if (type == 0u) {
      bgzf_drop(b, b.n & 7u);  // to the byte boundary
      bgzf_refill(b);
      if (b.n < 32u) return BGZF_E_IN_END;
      const uint32_t len = bgzf_peek(b, 16);
      bgzf_drop(b, 16);
      const uint32_t nlen = bgzf_peek(b, 16);
      bgzf_drop(b, 16);
      if (len != (nlen ^ 0xFFFFu)) return BGZF_E_STORED_LEN;
      b.p -= b.n >> 3;  // the whole bytes the bit buffer holds were read from here: give them back
      b.bits = 0;
      b.n = 0;
      if ((uint64_t)(b.end - b.p) < len) return BGZF_E_IN_END;
      if (len > isize - pos) return BGZF_E_OUT_OVER;
      if (len) out.stored(pos, b.p, len);
      b.p += len;
      pos += len;
    } else {
      bgzf_huff lit = bgzf_lit_huff(t), dist = bgzf_dist_huff(t);
      uint32_t mx = 0;
      if (type == 1u) {
        for (uint32_t s = 0; s < 288u; ++s) t.lengths[s] = (uint8_t)(s < 144u ? 8 : s < 256u ? 9 : s < 280u ? 7 : 8);
        for (uint32_t s = 0; s < 32u; ++s) t.lengths[288u + s] = 5;
        (void)bgzf_build(lit, t.lengths, 288u, false, false, &mx);
        (void)bgzf_build(dist, t.lengths + 288u, 32u, false, false, &mx);
      } else {
        if (b.n < 14u) return BGZF_E_IN_END;
        const uint32_t nlit = bgzf_peek(b, 5) + 257u;
        bgzf_drop(b, 5);
        const uint32_t ndist = bgzf_peek(b, 5) + 1u;
        bgzf_drop(b, 5);
        const uint32_t nclc = bgzf_peek(b, 4) + 4u;
        bgzf_drop(b, 4);
        if (nlit > 286u || ndist > 30u) return BGZF_E_HLIT_HDIST;
        const uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
        for (uint32_t i = 0; i < 19u; ++i) t.lengths[i] = 0;
        bgzf_refill(b);  // 19 * 3 = 57 bits: two refills
        for (uint32_t i = 0; i < 19u; ++i) {
          if (i == 10u) bgzf_refill(b);
          if (i < nclc) {
            if (b.n < 3u) return BGZF_E_IN_END;
            t.lengths[order[i]] = (uint8_t)bgzf_peek(b, 3);
            bgzf_drop(b, 3);
          }
        }
        bgzf_huff clc = bgzf_clc_huff(t);
        uint32_t st = bgzf_build(clc, t.lengths, 19u, false, false, &mx);  // (an incomplete code-length code is refused, as zlib does)
        if (st != BGZF_OK) return st;
        uint32_t idx = 0;
        const uint32_t total = nlit + ndist;
        while (idx < total) {  // every turn decodes a symbol: >= 1 bit
          bgzf_refill(b);
          const uint32_t sym = bgzf_decode(b, clc);
          if (sym >= 0x10000u) return sym >> 16;
          if (sym < 16u) {
            t.lengths[idx++] = (uint8_t)sym;  // (the code-length code's own lengths at [0, 19) are no longer needed: clc is built)
            continue;
          }
          uint32_t rep, val = 0;
          if (sym == 16u) {
            if (idx == 0) return BGZF_E_REP_NOPREV;
            if (b.n < 2u) return BGZF_E_IN_END;
            val = t.lengths[idx - 1u];
            rep = 3u + bgzf_peek(b, 2);
            bgzf_drop(b, 2);
          } else if (sym == 17u) {
            if (b.n < 3u) return BGZF_E_IN_END;
            rep = 3u + bgzf_peek(b, 3);
            bgzf_drop(b, 3);
          } else {
            if (b.n < 7u) return BGZF_E_IN_END;
            rep = 11u + bgzf_peek(b, 7);
            bgzf_drop(b, 7);
          }
          if (idx + rep > total) return BGZF_E_CL_RUN;
          RFX_BGZF_STAT(cl_run(sym, idx, rep, nlit));
          for (uint32_t i = 0; i < rep; ++i) t.lengths[idx++] = (uint8_t)val;
        }
        if (t.lengths[256] == 0) return BGZF_E_NO_EOB;
        // (the literal/length code first: its build touches neither the distance lengths nor the distance code's arrays,
        // which still hold the code-length code; the distance build then overwrites those)
        st = bgzf_build(lit, t.lengths, nlit, false, true, &mx);
        if (st != BGZF_OK) return st;
        RFX_BGZF_STAT(code_len(mx));
        st = bgzf_build(dist, t.lengths + nlit, ndist, true, true, &mx);
        if (st != BGZF_OK) return st;
        RFX_BGZF_STAT(code_len(mx));
        RFX_BGZF_STAT(dist_codes(t.dist_count, mx));
      }
      for (;;) {  // one literal/length symbol per turn: >= 1 bit
        // Refilled only when short (a refill is a dependent round trip to memory, a literal is ~8 bits): fewer than 15 bits
        // cannot hold every code; behind a length code its extra bits, a distance code and its extra bits are <= 33.
        if (b.n < 15u) bgzf_refill(b);
        const uint32_t sym = bgzf_decode(b, lit);
        if (sym >= 0x10000u) return sym >> 16;
        if (sym < 256u) {
          if (pos >= isize) return BGZF_E_OUT_OVER;
          out.literal(pos, sym);
          ++pos;
          continue;
        }
        if (sym == 256u) break;
        if (sym > 285u) return BGZF_E_LITLEN_SYM;
        if (b.n < 33u) bgzf_refill(b);
        uint32_t extra;
        uint32_t len = bgzf_len_base(sym, &extra);
        if (b.n < extra) return BGZF_E_IN_END;
        len += bgzf_peek(b, extra);
        bgzf_drop(b, extra);
        const uint32_t ds = bgzf_decode(b, dist);
        if (ds >= 0x10000u) return ds >> 16;
        if (ds > 29u) return BGZF_E_DIST_SYM;
        uint32_t d = bgzf_dist_base(ds, &extra);
        if (b.n < extra) return BGZF_E_IN_END;
        d += bgzf_peek(b, extra);
        bgzf_drop(b, extra);
        if (d > pos) return BGZF_E_DIST_FAR;
        if (len > isize - pos) return BGZF_E_OUT_OVER;
        RFX_BGZF_STAT(match(len, d));
        out.match(pos, len, d);
        pos += len;
      }
    }
    if (final_block) break;
  }
  out.end();
  if (pos != isize) return BGZF_E_OUT_SHORT;
  if ((b.n >> 3) + (uint64_t)(b.end - b.p) != 0) return BGZF_E_TRAILING;  // (the last byte's unused bits are padding)
  return BGZF_OK;
}
