// BAM record layout (section 4.2 of the SAM specification), written ONCE for host and device the way rfx_bgzf_core.h is:
// every function is RFX_BAM_HD, so the statements the kernels of rfx_bam.hip run are the statements
// tests/host/bam_harness.cpp runs under AddressSanitizer and UBSan.  Replaces the record framing `samtools view` does in
// front of PassThroughSamCheck (runRufus.sh:599, scripts/RunJellyForRUFUS.sh:28).
//
// A record at byte p of the inflated stream (little endian, at any residue mod 4):
//     p +  0  block_size u32   bytes of the record BEHIND this field: the next record starts at p + 4 + block_size
//     p +  4  refID i32        p +  8  pos i32          p + 12  l_read_name u8   p + 13  mapq u8    p + 14  bin u16
//     p + 16  n_cigar_op u16   p + 18  flag u16         p + 20  l_seq u32        p + 24  next_refID i32
//     p + 28  next_pos i32     p + 32  tlen i32         p + 36  read_name (NUL-terminated), cigar (4 B per op),
//     seq (4 bits per base, high nibble first, (l_seq + 1) / 2 bytes), qual (l_seq bytes), aux
//
// Bounds.  Every read goes through bam_u8, one byte at an index the caller has checked to lie in [0, end): bam_next and
// bam_valid check before they read, bam_plausible reads the name's last byte only where it lies in front of `end`.
// Nothing here writes.
//
// Termination.  bam_next(p) is p + 4 + block_size in 64 bits with block_size unsigned, so it is >= p + 4; it is BAM_STOP
// where p + 4 > end or the sum lies behind `end`.  A walk `while (p < limit && (nx = bam_next(p)) != BAM_STOP) p = nx`
// therefore stays in [0, end], advances by at least 4 per step and ends after at most end / 4 steps, whatever the bytes are.
#pragma once
#include <stdint.h>

#if defined(__HIP__)
#include <hip/hip_runtime.h>
#define RFX_BAM_HD __host__ __device__ __forceinline__
#else
#define RFX_BAM_HD inline
#endif
// Statistics hook of the host harness (which refusals and paths were reached); nothing in the library or the kernels.
#ifndef RFX_BAM_STAT
#define RFX_BAM_STAT(x) ((void)0)
#endif

enum bam_status : uint32_t {
  BAM_OK = 0,
  BAM_E_BLOCK_SIZE = 1,  // block_size < 32: the fixed fields do not fit
  BAM_E_READ_NAME = 2,   // l_read_name == 0 (the name holds at least its NUL)
  BAM_E_L_SEQ = 3,       // l_seq < 0
  BAM_E_FIELDS = 4,      // name + cigar + sequence + qualities do not fit block_size
  BAM_E_REF_ID = 5,      // refID outside [-1, n_ref)
  BAM_STATUS_COUNT = 6
};

inline const char* bam_status_text(uint32_t s) {
  static const char* const text[BAM_STATUS_COUNT] = {"ok",
                                                     "block_size below 32",
                                                     "l_read_name is 0",
                                                     "negative l_seq",
                                                     "name, cigar, sequence and qualities exceed block_size",
                                                     "refID outside the header's references"};
  return s < BAM_STATUS_COUNT ? text[s] : "unknown status";
}

constexpr uint64_t BAM_STOP = ~0ull;  // bam_next: the chain ends at p (no whole record starts there)
constexpr uint32_t BAM_FIXED = 36;    // block_size + the 32 bytes of fixed fields

RFX_BAM_HD uint32_t bam_u8(const uint8_t* b, uint64_t i) { return b[i]; }
RFX_BAM_HD uint32_t bam_u16(const uint8_t* b, uint64_t i) { return bam_u8(b, i) | bam_u8(b, i + 1) << 8; }
RFX_BAM_HD uint32_t bam_u32(const uint8_t* b, uint64_t i) {
  return bam_u8(b, i) | bam_u8(b, i + 1) << 8 | bam_u8(b, i + 2) << 16 | bam_u8(b, i + 3) << 24;
}

// ---- field decode: the caller has p + BAM_FIXED <= end (block_size alone: p + 4 <= end) ------------------------------
RFX_BAM_HD uint32_t bam_block_size(const uint8_t* b, uint64_t p) { return bam_u32(b, p); }
RFX_BAM_HD int32_t bam_ref_id(const uint8_t* b, uint64_t p) { return (int32_t)bam_u32(b, p + 4); }
RFX_BAM_HD int32_t bam_pos(const uint8_t* b, uint64_t p) { return (int32_t)bam_u32(b, p + 8); }
RFX_BAM_HD uint32_t bam_l_read_name(const uint8_t* b, uint64_t p) { return bam_u8(b, p + 12); }
RFX_BAM_HD uint32_t bam_n_cigar_op(const uint8_t* b, uint64_t p) { return bam_u16(b, p + 16); }
RFX_BAM_HD uint32_t bam_flag(const uint8_t* b, uint64_t p) { return bam_u16(b, p + 18); }
RFX_BAM_HD int32_t bam_l_seq(const uint8_t* b, uint64_t p) { return (int32_t)bam_u32(b, p + 20); }
RFX_BAM_HD int32_t bam_next_ref_id(const uint8_t* b, uint64_t p) { return (int32_t)bam_u32(b, p + 24); }
RFX_BAM_HD int32_t bam_next_pos(const uint8_t* b, uint64_t p) { return (int32_t)bam_u32(b, p + 28); }
RFX_BAM_HD uint64_t bam_seq_offset(const uint8_t* b, uint64_t p) {
  return p + BAM_FIXED + bam_l_read_name(b, p) + 4ull * bam_n_cigar_op(b, p);
}

// The start of the record behind the one at p, or BAM_STOP: no whole record lies at p of [0, end).
RFX_BAM_HD uint64_t bam_next(const uint8_t* b, uint64_t p, uint64_t end) {
  if (p + 4 > end) return BAM_STOP;
  const uint64_t nx = p + 4 + (uint64_t)bam_block_size(b, p);
  return nx > end ? BAM_STOP : nx;
}

// What a record on the TRUE chain must satisfy; the record is whole (bam_next(p) != BAM_STOP).  The fixed fields are read
// only behind the block_size check, which -- the record being whole -- puts them in front of `end`.
RFX_BAM_HD uint32_t bam_valid(const uint8_t* b, uint64_t p, int32_t n_ref) {
  const uint32_t bs = bam_block_size(b, p);
  if (bs < 32u) { RFX_BAM_STAT(refusal(BAM_E_BLOCK_SIZE)); return BAM_E_BLOCK_SIZE; }
  const uint32_t l_name = bam_l_read_name(b, p);
  if (l_name < 1u) { RFX_BAM_STAT(refusal(BAM_E_READ_NAME)); return BAM_E_READ_NAME; }
  const int32_t l_seq = bam_l_seq(b, p);
  if (l_seq < 0) { RFX_BAM_STAT(refusal(BAM_E_L_SEQ)); return BAM_E_L_SEQ; }
  const uint64_t need = 32ull + l_name + 4ull * bam_n_cigar_op(b, p) + ((uint64_t)l_seq + 1) / 2 + (uint64_t)l_seq;
  if (need > bs) { RFX_BAM_STAT(refusal(BAM_E_FIELDS)); return BAM_E_FIELDS; }
  const int32_t ref = bam_ref_id(b, p);
  if (ref < -1 || ref >= n_ref) { RFX_BAM_STAT(refusal(BAM_E_REF_ID)); return BAM_E_REF_ID; }
  return BAM_OK;
}

// bam_valid plus the cheap extras a guesser wants, for a candidate with p + BAM_FIXED <= end that need not be whole: the
// mate's reference in range, positions >= -1, the name's last byte a NUL (where that byte lies in front of `end`).
// Used ONLY to guess where a tile's first record starts: no result depends on it.
RFX_BAM_HD bool bam_plausible(const uint8_t* b, uint64_t p, uint64_t end, int32_t n_ref) {
  const uint32_t bs = bam_block_size(b, p);
  if (bs < 32u) return false;
  const uint32_t l_name = bam_l_read_name(b, p);
  const int32_t l_seq = bam_l_seq(b, p);
  if (l_name < 1u || l_seq < 0) return false;
  if (32ull + l_name + 4ull * bam_n_cigar_op(b, p) + ((uint64_t)l_seq + 1) / 2 + (uint64_t)l_seq > bs) return false;
  const int32_t ref = bam_ref_id(b, p), nref = bam_next_ref_id(b, p);
  if (ref < -1 || ref >= n_ref || nref < -1 || nref >= n_ref) return false;
  if (bam_pos(b, p) < -1 || bam_next_pos(b, p) < -1) return false;
  const uint64_t nul = p + BAM_FIXED + l_name - 1;
  return nul >= end || bam_u8(b, nul) == 0;
}

// The guess: candidate c looks like a record start when it is plausible and its next two chain steps are plausible too,
// or reach the end of the bytes (the last record of an arena is rarely whole).
RFX_BAM_HD bool bam_guess_ok(const uint8_t* b, uint64_t c, uint64_t end, int32_t n_ref) {
  uint64_t p = c;
  for (int step = 0; step < 3; ++step) {
    if (p + BAM_FIXED > end) return step > 0;  // the end reached behind at least one plausible record
    if (!bam_plausible(b, p, end, n_ref)) return false;
    const uint64_t nx = p + 4 + (uint64_t)bam_block_size(b, p);
    if (nx > end) return true;  // a record cut by the end
    p = nx;
  }
  return true;
}

// ---- the region test of `samtools view X.bam CHR:BEG-END` (rfx_bam_set_region) ----------------------------------------
// Both run on a record bam_valid accepts: its cigar lies inside the record, and every byte is read through bam_u8.
// bam_end_pos: pos + rlen in 64 bits, rlen = the lengths of the M, D, N, = and X operations (codes 0, 2, 3, 7, 8: the mask
// 0x18D) added up; 1 for an unmapped record (flag 4), one without an operation and one whose operations consume nothing.
// n_cigar_op <= 65535 and a length < 2^28, so the sum stays below 2^44.
RFX_BAM_HD int64_t bam_end_pos(const uint8_t* b, uint64_t p) {
  const int64_t pos = bam_pos(b, p);
  const uint32_t n_op = bam_n_cigar_op(b, p);
  if ((bam_flag(b, p) & 4u) || n_op == 0) return pos + 1;
  const uint64_t cigar = p + BAM_FIXED + bam_l_read_name(b, p);
  int64_t rlen = 0;
  for (uint32_t i = 0; i < n_op; ++i) {
    const uint32_t v = bam_u32(b, cigar + 4ull * i);
    if ((0x18Du >> (v & 15u)) & 1u) rlen += (int64_t)(v >> 4);
  }
  return pos + (rlen ? rlen : 1);
}
// the record overlaps [beg, end) of reference tid
RFX_BAM_HD bool bam_in_region(const uint8_t* b, uint64_t p, int32_t tid, int64_t beg, int64_t end) {
  if (bam_ref_id(b, p) != tid || (int64_t)bam_pos(b, p) >= end) return false;
  return bam_end_pos(b, p) > beg;
}
// What every kernel of rfx_bam.hip calls a KEPT record r (at offset p): none of the excluded flags, and -- while the arena
// has a region (region != NULL: rfx_bam_set_region's byte per record) -- inside it.
RFX_BAM_HD bool bam_kept(const uint8_t* b, uint64_t p, uint32_t exclude, const uint8_t* region, uint64_t r) {
  return (bam_flag(b, p) & exclude) == 0 && (!region || region[r] != 0);
}

// One tile's walk: from `in` along bam_next until the offset is >= limit (the tile's end) or the chain ends.  Returns
// where it stands and adds the whole records it passed -- they START in [in, limit) -- to *count.  An entry that already
// lies behind the limit is passed through.  visit(p): called for every record passed (the kernels write and check it).
template <class Visit>
RFX_BAM_HD uint64_t bam_walk(const uint8_t* b, uint64_t in, uint64_t limit, uint64_t end, uint32_t* count, Visit& visit) {
  uint64_t p = in;
  uint32_t n = 0;
  while (p < limit) {
    const uint64_t nx = bam_next(b, p, end);
    if (nx == BAM_STOP) break;
    visit(p, n);
    ++n;
    p = nx;
  }
  *count = n;
  return p;
}
struct bam_no_visit {
  RFX_BAM_HD void operator()(uint64_t, uint32_t) {}
};

// ---- 4-bit bases -> a count block's code word -----------------------------------------------------------------------
// w[0 .. 3] = the 16 sequence bytes of one code word in stream order (byte i = bits 8 (i % 4) of w[i / 4]); nb <= 32 bases
// are taken, high nibble first.  What rfx_pack_reads(RFX_PACK_COUNT) makes of "=ACMGRSVTWYHKDBN"[nibble]: nibbles 1 / 2 /
// 4 / 8 are A / C / G / T (codes 0 .. 3, mask bit set), every other nibble is an invalid base (code 0, mask bit clear).
RFX_BAM_HD void bam_pack_word(const uint32_t w[4], uint32_t nb, uint64_t* code, uint32_t* mask) {
  uint64_t c = 0;
  uint32_t m = 0;
  for (uint32_t i = 0; i < 32u; ++i) {
    if (i < nb) {
      const uint32_t byte = (w[i >> 3] >> (8u * ((i >> 1) & 3u))) & 255u;
      const uint32_t nib = (i & 1u) ? (byte & 15u) : (byte >> 4);
      const uint32_t ok = (0x0116u >> nib) & 1u;  // 1, 2, 4, 8
      c |= (uint64_t)(ok ? (nib >> 1) - (nib >> 3) : 0u) << (2u * i);
      m |= ok << i;
    }
  }
  *code = c;
  *mask = m;
}

// ---- the stranded filter form of a record (rfx_bam_parse_filter) --------------------------------------------------------
// What rfx_pack_reads(RFX_PACK_FILTER) makes of the record as `samtools view | PassThroughSamCheck.stranded` prints it
// (src/PassThroughSamCheck.stranded.cpp:184-223): SEQ = "=ACMGRSVTWYHKDBN"[nibble] (`*` for l_seq == 0), QUAL = 33 +
// min(q, 93) per base (`*` for l_seq == 0 or qual[0] == 0xFF); a record with flag & 16 has its sequence reversed and
// complemented, every base that is none of A C G T N VANISHES (the read gets shorter), and its whole quality string is
// reversed: position j of the read meets reversed quality j.  The caller has a record bam_valid accepts, so sequence and
// qualities lie inside the record.
RFX_BAM_HD uint32_t bam_nibble(const uint8_t* b, uint64_t seq, uint32_t i) {
  const uint32_t byte = bam_u8(b, seq + (i >> 1));
  return (i & 1u) ? (byte & 15u) : (byte >> 4);
}
RFX_BAM_HD uint32_t bam_survives(uint32_t nib) { return (0x8116u >> nib) & 1u; }  // A C G T N: nibbles 1 2 4 8 15
// bases of the printed read: forward max(l_seq, 1) (`*` is one base); reverse the surviving nibbles (`*` vanishes: 0)
RFX_BAM_HD uint32_t bam_filter_len(const uint8_t* b, uint64_t p) {
  const uint32_t l_seq = (uint32_t)bam_l_seq(b, p);
  if (!(bam_flag(b, p) & 16u)) return l_seq ? l_seq : 1u;
  const uint64_t seq = bam_seq_offset(b, p);
  uint32_t n = 0;
  for (uint32_t i = 0; i < l_seq; ++i) n += bam_survives(bam_nibble(b, seq, i));
  return n;
}
// Code word j of the printed read of `len` bases (bam_filter_len) and its `good` mask: code = A C G T -> 0 .. 3, anything
// else 0; good = (qualchar - 33 >= min_q) && base != 'N', a position without a quality character reading as '\0'
// (rfx_pack_reads; src/RUFUS.Filter.cpp:205).  A reverse read with vanished bases is compacted by a walk from the
// sequence's end (rare: one walk per word).
RFX_BAM_HD void bam_filter_word(const uint8_t* b, uint64_t p, uint32_t j, uint32_t len, int min_q, uint64_t* code, uint32_t* good) {
  const uint32_t l_seq = (uint32_t)bam_l_seq(b, p);
  const bool rev = (bam_flag(b, p) & 16u) != 0;
  const uint64_t seq = bam_seq_offset(b, p), qual = seq + (l_seq + 1u) / 2u;
  const bool no_qual = l_seq == 0 || bam_u8(b, qual) == 0xFFu;
  const uint32_t first = j * 32u, nb = len - first < 32u ? len - first : 32u;
  uint64_t c = 0;
  uint32_t g = 0;
  // s: the source nibble of read position first + i.  Forward: the position; reverse: from the end, over survivors only
  uint32_t s = rev ? l_seq : 0u, skipped = 0;
  const bool compact = rev && len != l_seq;
  if (rev && !compact) s = l_seq - first;
  for (uint32_t i = 0; i < nb; ++i) {
    const uint32_t pos = first + i;
    uint32_t nib = 0;  // (`*`: a base that is none of A C G T N)
    if (rev) {
      if (compact) {
        while (skipped <= pos) {  // (ends: the read has len > pos survivors)
          --s;
          skipped += bam_survives(bam_nibble(b, seq, s));
        }
      } else {
        --s;
      }
      nib = bam_nibble(b, seq, s);
    } else if (l_seq) {
      nib = bam_nibble(b, seq, pos);
    }
    const uint32_t acgt = (0x0116u >> nib) & 1u;
    const uint32_t fwd = (nib >> 1) - (nib >> 3);
    c |= (uint64_t)(acgt ? (rev ? 3u - fwd : fwd) : 0u) << (2u * i);
    // the quality character: `*` is ONE character; a reverse record's string is reversed whole
    int q = 0;
    if (no_qual) q = pos == 0 ? '*' : 0;
    else if (pos < l_seq) {
      const uint32_t v = bam_u8(b, qual + (rev ? l_seq - 1u - pos : pos));
      q = 33 + (int)(v < 93u ? v : 93u);
    }
    g |= (uint32_t)(q - 33 >= min_q && nib != 15u) << i;
  }
  *code = c;
  *good = g;
}

// The printed QNAME: the name field's bytes up to its first NUL (l_read_name counts the NUL; a field without one: all of
// it).  bam_name_hash: FNV-1a over those bytes, then the splitmix64 finaliser.  Only which records are LOOKED AT depends on
// it (rfx_bam_mark_names): names are compared as bytes wherever a result is decided.
RFX_BAM_HD uint32_t bam_name_len(const uint8_t* b, uint64_t p) {
  const uint32_t l = bam_l_read_name(b, p);
  uint32_t n = 0;
  while (n < l && bam_u8(b, p + BAM_FIXED + n) != 0) ++n;
  return n;
}
RFX_BAM_HD uint64_t bam_name_hash(const uint8_t* b, uint64_t p) {
  const uint32_t l = bam_l_read_name(b, p);
  uint64_t h = 0xCBF29CE484222325ull;
  for (uint32_t i = 0; i < l; ++i) {
    const uint32_t ch = bam_u8(b, p + BAM_FIXED + i);
    if (ch == 0) break;
    h = (h ^ ch) * 0x100000001B3ull;
  }
  h += 0x9E3779B97F4A7C15ull;
  h = (h ^ (h >> 30)) * 0xBF58476D1CE4E5B9ull;
  h = (h ^ (h >> 27)) * 0x94D049BB133111EBull;
  return h ^ (h >> 31);
}
