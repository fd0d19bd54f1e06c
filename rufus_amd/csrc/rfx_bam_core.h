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
