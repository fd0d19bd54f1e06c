// Plain-gzip decoder core: a deflate stream (RFC 1951) WITHOUT BGZF's framing, cut speculatively, decoded with an unknown
// 32 KiB history and then repaired.  Replaces the inflate of `zcat F.fastq.gz | ...` (runRufus.sh:157-160, :229-232,
// :974-977) for the files a sequencer or an archive hands out.  Bit reader, Huffman tables, the length and distance tables
// and the CRC shift-and-combine are rfx_bgzf_core.h's; that file is untouched (the dynamic-header parse is written out a
// second time here, gz_dyn_header, so that k_bgzf_inflate compiles to what it compiled to before).
//
// Written ONCE, for host and device, as rfx_bgzf_core.h is: the kernels of rfx_gzip.hip and tests/host/gzip_harness.cpp
// (AddressSanitizer, UBSan) run the same statements; the chain rule that makes the speculation safe (gz_append below, host
// only) is a template over the backend that finds, walks and inflates -- the kernels in the library, serial loops in the
// harness.
//
//   gz_member_header  RFC 1952 header (FEXTRA / FNAME / FCOMMENT / FHCRC) -> the first deflate byte.  Host only.
//   gz_prefilter      registers only: the 17 header bits of a non-final dynamic block and Kraft equality of the <= 19
//                     three-bit code-length lengths (sum of 2^(7 - len) = 128).  ~1 bit offset in 1000 passes.
//   gz_probe          the strict header check at a bit offset: BFINAL = 0, BTYPE = 2 and gz_dyn_header(strict) -- the
//                     statements the decoder runs on a real header; strict only refuses the single-code literal/length
//                     code a decoder must accept and a compressor never writes for text.
//   gz_run<Out>       the block loop from a start bit: blocks are decoded until one ends at or beyond a stop bit, or the
//                     final block ends, or the input ends (BGZF_E_IN_END: a status of its own, the driver waits for more
//                     input on it).  With gz_null_out it is the WALK: nothing is stored, bytes are counted -- the size of a
//                     block's output does not depend on the history, so sizes are known before anything is stored.
//   gz_serial16 / the kernel's wave policy: 16-bit output.  A value below 256 is a byte; 0x8000 | w is "byte w of the 32 KiB
//                     that precede this chunk's first output byte".  A match whose source index j = pos - d + i mod d is
//                     negative stores 0x8000 | (32768 + j); a match that copies markers copies them.  d <= 32768 by the
//                     format (distance symbol 29 with 13 extra bits), so 32768 + j >= 0 and no index outside the chunk's
//                     own buffer is read or written, whatever the input says.  BGZF_E_DIST_FAR becomes the rule that a
//                     marker is illegal in the first chunk of a member.
//   gz_history        a marker resolved against (window buffer ++ this batch's bytes).
//
// Bounds.  Input is read only through bgzf_bits over [p, end) and, for a stored run, a range checked to lie inside it.  The
// policy is called only with pos + len <= max_out (the chunk's size as the walk reported it).
//
// Termination.  Same rule as the BGZF core: every loop in this file runs a number of times fixed by a table size (<= 1024
// iterations), or consumes at least one input bit, or emits at least one output byte, or returns.  gz_run therefore ends
// after at most 8 * (end - p) + max_out steps; the chain rule's rounds each confirm, drop or insert a chunk.
#pragma once
#include "rfx_bgzf_core.h"

#include <string>
#include <vector>

constexpr uint32_t GZ_WINDOW = 32768;
constexpr uint64_t GZ_NO_STOP = ~0ull;

inline const char* gz_status_text(uint32_t s) {
  return s == BGZF_E_DIST_FAR ? "distance reaches before the member's first byte" : bgzf_status_text(s);
}

// 0: a whole header lies in [b, b + avail), *len = its bytes (the first deflate byte);  1: a valid beginning, not whole;
// -1: not a gzip member (magic, CM other than 8, a reserved FLG bit).
inline int gz_member_header(const uint8_t* b, uint64_t avail, uint64_t* len) {
  static const uint8_t magic[3] = {0x1f, 0x8b, 0x08};
  for (uint64_t i = 0; i < 3 && i < avail; ++i)
    if (b[i] != magic[i]) return -1;
  if (avail > 3 && (b[3] & 0xE0u)) return -1;
  if (avail < 10) return 1;
  const uint32_t flg = b[3];
  uint64_t at = 10;
  if (flg & 4u) {  // FEXTRA
    if (avail < at + 2) return 1;
    at += 2 + (b[at] | (uint64_t)b[at + 1] << 8);
    if (avail < at) return 1;
  }
  for (uint32_t bit = 8u; bit <= 16u; bit <<= 1)  // FNAME, FCOMMENT: zero-terminated
    if (flg & bit) {
      while (at < avail && b[at]) ++at;
      if (at >= avail) return 1;
      ++at;
    }
  if (flg & 2u) at += 2;  // FHCRC
  if (avail < at) return 1;
  *len = at;
  return 0;
}

// ---- a bit reader placed at a bit offset of [p, end) ---------------------------------------------------------------------
RFX_BGZF_HD void gz_bits_at(bgzf_bits& b, const uint8_t* p, const uint8_t* end, uint64_t bit) {  // (bit >> 3) <= end - p
  bgzf_bits_init(b, p + (bit >> 3), end);
  bgzf_refill(b);
  const uint32_t k = (uint32_t)bit & 7u;
  if (b.n >= k) {
    bgzf_drop(b, k);
  } else {
    b.bits = 0;
    b.n = 0;
  }
}
RFX_BGZF_HD uint64_t gz_bit_pos(const bgzf_bits& b, const uint8_t* p) { return (uint64_t)(b.p - p) * 8u - b.n; }

// ---- stage one of the finder: registers only ---------------------------------------------------------------------------
// lo = the 64 stream bits from the candidate's first bit on, hi = the 64 behind them.
RFX_BGZF_HD bool gz_prefilter(uint64_t lo, uint64_t hi) {
  const uint32_t h = (uint32_t)lo & 0x1FFFFu;
  if ((h & 7u) != 4u) return false;  // BFINAL = 0, BTYPE = 2
  if (((h >> 3) & 31u) > 29u || ((h >> 8) & 31u) > 29u) return false;
  const uint32_t nclc = ((h >> 13) & 15u) + 4u;
  const uint64_t y = lo >> 17 | hi << 47;  // 19 * 3 = 57 bits
  uint32_t sum = 0;
  for (uint32_t i = 0; i < 19u; ++i) {
    const uint32_t l = (uint32_t)(y >> (3u * i)) & 7u;
    if (i < nclc && l) sum += 128u >> l;
  }
  return sum == 128u;
}
// The 128 stream bits at `bit` of [p, end), bytes beyond the end read as zero (host side and the tail of the kernel's).
RFX_BGZF_HD void gz_bits128(const uint8_t* p, const uint8_t* end, uint64_t bit, uint64_t* lo, uint64_t* hi) {
  const uint8_t* q = p + (bit >> 3);
  uint64_t w[3] = {0, 0, 0};
  for (uint32_t i = 0; i < 17u; ++i)
    if (q + i < end) w[i >> 3] |= (uint64_t)q[i] << (8u * (i & 7u));
  const uint32_t s = (uint32_t)bit & 7u;
  *lo = s ? w[0] >> s | w[1] << (64u - s) : w[0];
  *hi = s ? w[1] >> s | w[2] << (64u - s) : w[1];
}

// ---- a dynamic block's header, behind its three type bits: the tables of its two codes ------------------------------------
// (rfx_bgzf_core.h's statements; strict: the literal/length code must be complete.)
RFX_BGZF_HD uint32_t gz_dyn_header(bgzf_bits& b, bgzf_tables& t, bool strict) {
  bgzf_huff lit = bgzf_lit_huff(t), dist = bgzf_dist_huff(t);
  uint32_t mx = 0;
  bgzf_refill(b);
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
  uint32_t st = bgzf_build(clc, t.lengths, 19u, false, false, &mx);
  if (st != BGZF_OK) return st;
  uint32_t idx = 0;
  const uint32_t total = nlit + ndist;
  while (idx < total) {  // every turn decodes a symbol: >= 1 bit
    bgzf_refill(b);
    const uint32_t sym = bgzf_decode(b, clc);
    if (sym >= 0x10000u) return sym >> 16;
    if (sym < 16u) {
      t.lengths[idx++] = (uint8_t)sym;
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
    for (uint32_t i = 0; i < rep; ++i) t.lengths[idx++] = (uint8_t)val;
  }
  if (t.lengths[256] == 0) return BGZF_E_NO_EOB;
  st = bgzf_build(lit, t.lengths, nlit, false, !strict, &mx);
  if (st != BGZF_OK) return st;
  return bgzf_build(dist, t.lengths + nlit, ndist, true, true, &mx);
}

// Stage two of the finder: does a non-final dynamic block with a valid header start at `bit`?
RFX_BGZF_HD bool gz_probe(const uint8_t* p, const uint8_t* end, uint64_t bit, bgzf_tables& t) {
  bgzf_bits b;
  gz_bits_at(b, p, end, bit);
  if (b.n < 3u || bgzf_peek(b, 3) != 4u) return false;
  bgzf_drop(b, 3);
  return gz_dyn_header(b, t, true) == BGZF_OK;
}

// ---- the block loop ----------------------------------------------------------------------------------------------------
struct gz_result {
  uint64_t end_bit;    // where the last decoded block ends (status BGZF_OK)
  uint64_t out_bytes;  // bytes the decoded blocks inflate to
  uint32_t final_seen, status;
};

struct gz_null_out {  // the walk: nothing is stored
  RFX_BGZF_HD void literal(uint64_t, uint32_t) {}
  RFX_BGZF_HD void match(uint64_t, uint32_t, uint32_t) {}
  RFX_BGZF_HD void stored(uint64_t, const uint8_t*, uint32_t) {}
  RFX_BGZF_HD void end() {}
};

// One block behind its three type bits.  `first`: the chunk begins a member, so a distance beyond `pos` is an error.
template <class Out>
RFX_BGZF_HD uint32_t gz_block(bgzf_bits& b, uint32_t type, bool first, uint64_t max_out, bgzf_tables& t, Out& out, uint64_t& pos) {
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
    if (len > max_out - pos) return BGZF_E_OUT_OVER;
    if (len) out.stored(pos, b.p, len);
    b.p += len;
    pos += len;
    return BGZF_OK;
  }
  bgzf_huff lit = bgzf_lit_huff(t), dist = bgzf_dist_huff(t);
  if (type == 1u) {
    uint32_t mx = 0;
    for (uint32_t s = 0; s < 288u; ++s) t.lengths[s] = (uint8_t)(s < 144u ? 8 : s < 256u ? 9 : s < 280u ? 7 : 8);
    for (uint32_t s = 0; s < 32u; ++s) t.lengths[288u + s] = 5;
    (void)bgzf_build(lit, t.lengths, 288u, false, false, &mx);
    (void)bgzf_build(dist, t.lengths + 288u, 32u, false, false, &mx);
  } else {
    const uint32_t st = gz_dyn_header(b, t, false);
    if (st != BGZF_OK) return st;
  }
  for (;;) {  // one literal/length symbol per turn: >= 1 bit
    if (b.n < 15u) bgzf_refill(b);
    const uint32_t sym = bgzf_decode(b, lit);
    if (sym >= 0x10000u) return sym >> 16;
    if (sym < 256u) {
      if (pos >= max_out) return BGZF_E_OUT_OVER;
      out.literal(pos, sym);
      ++pos;
      continue;
    }
    if (sym == 256u) return BGZF_OK;
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
    bgzf_drop(b, extra);  // (d <= 24577 + 8191 = GZ_WINDOW)
    if (first && d > pos) return BGZF_E_DIST_FAR;
    if (len > max_out - pos) return BGZF_E_OUT_OVER;
    out.match(pos, len, d);
    pos += len;
  }
}

template <class Out>
RFX_BGZF_HD void gz_run(const uint8_t* p, const uint8_t* end, uint64_t start_bit, uint64_t stop_bit, bool first, uint64_t max_out,
                        bgzf_tables& t, Out& out, gz_result& r) {
  bgzf_bits b;
  gz_bits_at(b, p, end, start_bit);
  uint64_t pos = 0;
  uint32_t st = BGZF_OK, fin = 0;
  for (;;) {  // one deflate block per turn: >= 3 bits
    bgzf_refill(b);
    if (b.n < 3u) {
      st = BGZF_E_IN_END;
      break;
    }
    const uint32_t final_block = bgzf_peek(b, 1), type = bgzf_peek(b, 3) >> 1;
    bgzf_drop(b, 3);
    st = gz_block(b, type, first, max_out, t, out, pos);
    if (st != BGZF_OK) break;
    if (final_block) {
      fin = 1;
      break;
    }
    if (gz_bit_pos(b, p) >= stop_bit) break;
  }
  out.end();
  r.end_bit = gz_bit_pos(b, p);
  r.out_bytes = pos;
  r.final_seen = fin;
  r.status = st;
}

// The 16-bit output policy, serial (the harness; the kernel's spreads the same stores over a wave).
struct gz_serial16 {
  uint16_t* out;
  void literal(uint64_t pos, uint32_t byte) { out[pos] = (uint16_t)byte; }
  void match(uint64_t pos, uint32_t len, uint32_t dist) {
    for (uint32_t i = 0; i < len; ++i) {
      const int64_t j = (int64_t)pos - (int64_t)dist + (int64_t)(i % dist);
      out[pos + i] = j < 0 ? (uint16_t)(0x8000u | (uint32_t)((int64_t)GZ_WINDOW + j)) : out[j];
    }
  }
  void stored(uint64_t pos, const uint8_t* src, uint32_t n) {
    for (uint32_t i = 0; i < n; ++i) out[pos + i] = src[i];
  }
  void end() {}
};

// Byte w of the 32 KiB in front of the chunk whose first byte is byte `chunk_off` of the batch: the stream's last 32 KiB
// before the batch are `win`, the batch's own bytes `batch_out` (resolved there: see k_gz_windows).
RFX_BGZF_HD uint8_t gz_history(const uint8_t* batch_out, const uint8_t* win, uint64_t chunk_off, uint32_t w) {
  const uint64_t k = chunk_off + w;  // index into win ++ batch_out
  return k < GZ_WINDOW ? win[k] : batch_out[k - GZ_WINDOW];
}
RFX_BGZF_HD uint8_t gz_resolve16(uint32_t v, const uint8_t* batch_out, const uint8_t* win, uint64_t chunk_off) {
  return v < 0x8000u ? (uint8_t)v : gz_history(batch_out, win, chunk_off, v & 0x7FFFu);
}

// ---- the chain rule (host only) ------------------------------------------------------------------------------------------
// One chunk of the presented input: bits [start, end) once walked; stop = the next chunk's start at the time of the walk.
struct gz_chunk {
  uint64_t start, stop;
  uint32_t first, walked;
  gz_result res;
};

// What lives from call to call.
struct gz_stream {
  uint32_t chunk_bytes = 1u << 16;  // the nominal chunk: a power of two (RFX_GZIP_CHUNK; 64 KiB: profiles/gzip_inflate.txt)
  int e_format = -1;                // what gz_append returns for a malformed file (msg says what)
  uint32_t bit = 0;                 // the stream goes on at this bit of the next presented byte
  int phase = 0;                    // 0: a member header (or the file's end) comes next; 1: deflate blocks; 2: the trailer
  bool first = true;                // the next chunk is the first of its member
  uint32_t crc_reg = 0xFFFFFFFFu;   // the member's CRC register so far
  uint64_t isize = 0;               // the member's bytes so far
  uint64_t member = 0, chunk_no = 0;
  uint64_t total_in = 0;            // compressed bytes done with, over all calls
  uint64_t need = 0;                // after a call that returned 0 with nothing consumed: the room the next chunk wants
  uint64_t stats[8] = {0, 0, 0, 0, 0, 0, 0, 0};  // found, confirmed, dropped, inserted, rounds, members, batches, bytes out
  std::vector<uint64_t> starts;     // every confirmed chunk's start, as a bit offset in the whole compressed stream
  std::string msg;
};

// Backend:
//   int find(uint64_t first_boundary, uint32_t chunk_bytes, std::vector<uint64_t>& cand)
//        for every boundary first_boundary + k * chunk_bytes < n: the first bit at or behind it, and before the next
//        boundary, where gz_probe passes -- ascending; boundaries without one add nothing
//   int walk(std::vector<gz_chunk>& list, const std::vector<uint32_t>& which)     list[i].res for i in which
//   int inflate(const gz_chunk* c, size_t n, uint64_t total, uint32_t* crc_reg)   the chunks' bytes appended to the arena,
//        crc_reg[i] = bgzf_crc_update(0, chunk i's bytes)
//   uint64_t room(), cap()
// (0 or a negative error that gz_append hands on.)
//
// Appends what [host, host + n) inflates to, as far as whole confirmed chunks go and the arena has room; returns the bytes
// appended or a negative error, *consumed = the whole bytes done with (S.bit: the bits of the next byte that are done too).
template <class Backend>
long gz_append(gz_stream& S, Backend& B, const uint8_t* host, uint64_t n, bool eof, uint64_t* consumed) {
  auto fail = [&](const std::string& what) -> long {
    S.msg = "rfx_gzip: " + what;
    return S.e_format;
  };
  auto chunk_fail = [&](uint64_t c, uint32_t st) -> long {
    return fail("member " + std::to_string(S.member - 1) + ", chunk " + std::to_string(c) + ": " + gz_status_text(st));
  };
  *consumed = 0;
  S.need = 0;
  uint64_t pos = 0, appended = 0;  // pos: bytes done with (plus S.bit bits)
  bool have_cand = false;
  std::vector<gz_chunk> list;  // behind the chain's head: the finder's candidates, ascending; their walks stay valid
  auto done = [&]() -> long {
    *consumed = pos;
    S.total_in += pos;
    return (long)appended;
  };
  for (;;) {
    if (S.phase == 0) {
      if (pos == n) {
        if (eof && S.member == 0) return fail("no gzip member");
        return done();
      }
      uint64_t hl = 0;
      const int h = gz_member_header(host + pos, n - pos, &hl);
      if (h < 0) return fail("member " + std::to_string(S.member) + ": no gzip member header (magic, CM or a reserved FLG bit)");
      if (h > 0) {
        if (eof) return fail("member " + std::to_string(S.member) + ": the header is cut off");
        return done();
      }
      pos += hl;
      S.bit = 0;
      S.phase = 1;
      S.first = true;
      S.crc_reg = 0xFFFFFFFFu;
      S.isize = 0;
      S.chunk_no = 0;
      ++S.member;
      ++S.stats[5];
    }
    if (S.phase == 2) {
      if (n - pos < 8) {
        if (eof) return fail("member " + std::to_string(S.member - 1) + ": the trailer is cut off");
        return done();
      }
      const uint8_t* ft = host + pos;
      const uint32_t crc = ft[0] | (uint32_t)ft[1] << 8 | (uint32_t)ft[2] << 16 | (uint32_t)ft[3] << 24;
      const uint32_t isz = ft[4] | (uint32_t)ft[5] << 8 | (uint32_t)ft[6] << 16 | (uint32_t)ft[7] << 24;
      if (~S.crc_reg != crc) return fail("member " + std::to_string(S.member - 1) + ": CRC mismatch");
      if ((uint32_t)S.isize != isz) return fail("member " + std::to_string(S.member - 1) + ": ISIZE mismatch");
      pos += 8;
      S.phase = 0;
      continue;
    }
    // ---- deflate blocks from bit `start` of the presented bytes
    const uint64_t start = pos * 8u + S.bit;
    if (pos >= n) {
      if (eof) return chunk_fail(S.chunk_no, BGZF_E_IN_END);
      return done();
    }
    if (!have_cand) {
      have_cand = true;
      const uint64_t cb = S.chunk_bytes;
      std::vector<uint64_t> cand;
      if (const int rc = B.find((cb - S.total_in % cb) % cb, S.chunk_bytes, cand)) return rc;
      S.stats[0] += cand.size();
      for (uint64_t c : cand) list.push_back(gz_chunk{c, 0, 0u, 0u, gz_result{0, 0, 0, 0}});
    }
    {  // what lies in front of the head (a trailer's and a header's bytes) is no chunk start; the head itself is one
      size_t k = 0;
      while (k < list.size() && list[k].start < start) ++k;
      S.stats[2] += k;
      list.erase(list.begin(), list.begin() + (long)k);
      if (list.empty() || list[0].start != start) list.insert(list.begin(), gz_chunk{start, 0, 0u, 0u, gz_result{0, 0, 0, 0}});
      if (S.first && !list[0].first) {
        list[0].first = 1u;
        list[0].walked = 0u;
      }
    }
    // rounds: walk what has not been walked, then confirm along the chain
    size_t conf = 0;  // list[0 .. conf] are confirmed (list[conf] the last of them)
    bool ended = false, exhausted = false;
    while (!ended && !exhausted) {
      std::vector<uint32_t> which;
      for (size_t i = 0; i < list.size(); ++i) {
        const uint64_t stop = i + 1 < list.size() ? list[i + 1].start : GZ_NO_STOP;
        // (a walk that stopped behind a block at or beyond its stop is also the walk to any stop in (its last block's
        // start, its end]; only an unwalked chunk is walked: the chain below re-derives the rest from the end bits)
        if (!list[i].walked) {
          list[i].stop = stop;
          which.push_back((uint32_t)i);
        }
      }
      if (!which.empty()) {
        if (const int rc = B.walk(list, which)) return rc;
        for (uint32_t i : which) list[i].walked = 1u;
        ++S.stats[4];
      }
      for (;;) {
        gz_chunk& c = list[conf];
        if (c.res.status == BGZF_E_IN_END) {
          exhausted = true;
          break;
        }
        if (c.res.status != BGZF_OK) return chunk_fail(S.chunk_no + conf, c.res.status);
        if (c.res.final_seen) {
          ended = true;
          break;
        }
        size_t nx = conf + 1;
        size_t k = nx;
        while (k < list.size() && list[k].start < c.res.end_bit) ++k;  // candidates inside this chunk's blocks were false
        S.stats[2] += k - nx;
        list.erase(list.begin() + (long)nx, list.begin() + (long)k);
        if (nx < list.size() && list[nx].start == c.res.end_bit) {
          conf = nx;
          continue;
        }
        // the chunk ended in front of the next candidate (it was walked to a stop that has been dropped since), or there
        // is none: a chunk that starts at its end is inserted and walked
        list.insert(list.begin() + (long)nx, gz_chunk{c.res.end_bit, 0, 0u, 0u, gz_result{0, 0, 0, 0}});
        ++S.stats[3];
        conf = nx;
        break;  // (unwalked: the next round)
      }
    }
    // list[0 .. whole) are whole confirmed chunks
    const size_t whole = ended ? conf + 1 : conf;
    if (exhausted && eof) return chunk_fail(S.chunk_no + conf, BGZF_E_IN_END);
    size_t take = 0;
    uint64_t total = 0;
    const uint64_t room = B.room();
    while (take < whole && list[take].res.out_bytes <= room - total) total += list[take++].res.out_bytes;
    if (take) {
      std::vector<uint32_t> regs(take, 0u);
      if (const int rc = B.inflate(list.data(), take, total, regs.data())) return rc;
      for (size_t i = 0; i < take; ++i) {
        const uint64_t len = list[i].res.out_bytes;
        for (uint64_t left = len; left;) {  // (the shift takes 32 bits of length)
          const uint32_t step = (uint32_t)(left < 0x80000000ull ? left : 0x80000000ull);
          S.crc_reg = bgzf_crc_shift(S.crc_reg, step);
          left -= step;
        }
        S.crc_reg ^= regs[i];
        S.isize += len;
        S.starts.push_back((S.total_in + (list[i].start >> 3)) * 8u + (list[i].start & 7u));
      }
      S.first = false;
      S.chunk_no += take;
      S.stats[1] += take;
      ++S.stats[6];
      S.stats[7] += total;
      appended += total;
    }
    if (take < whole) {  // the arena is full
      const uint64_t want = list[take].res.out_bytes;
      if (want > B.cap())
        return fail("member " + std::to_string(S.member - 1) + ", chunk " + std::to_string(S.chunk_no) + ": a chunk of " +
                    std::to_string(want) + " inflated bytes does not fit an empty text arena");
      pos = list[take].start >> 3;
      S.bit = (uint32_t)list[take].start & 7u;
      S.need = want;
      return done();
    }
    if (ended) {
      pos = (list[conf].res.end_bit + 7u) >> 3;
      S.bit = 0;
      S.phase = 2;
      list.erase(list.begin(), list.begin() + (long)whole);
      continue;
    }
    // exhausted: the chunk at list[conf] and everything behind it wait for the next call
    pos = list[conf].start >> 3;
    S.bit = (uint32_t)list[conf].start & 7u;
    return done();
  }
}
