// FASTA text -> the reads of a packed block: the rule, written ONCE for host and device the way rfx_bgzf_core.h and
// rfx_bam_core.h are: every function is RFX_FASTA_HD, so the statements the kernels of rfx_fasta.hip run are the statements
// tests/host/fasta_harness.cpp runs under AddressSanitizer and UBSan.  Replaces, for FASTA, the text parser of
// jf/include/jellyfish/mer_overlap_sequence_parser.hpp:124-251 (rfxcli::parse_sequences, tools.parse_sequences) and the
// base table of jf/include/jellyfish/mer_dna.hpp:46-63.
//
// The rule.  A line ends at '\n' (only '\n' is stripped: a '\r' stays a base); the text's last line may lack it.  A line
// is a HEADER when it is non-empty and its first byte is '>' -- a '>' anywhere else is a base.  A record is a header and
// every line up to the next header or the end of the text; its sequence is the bytes of those lines without the '\n'.
// Empty lines add nothing; a header directly followed by a header is a read of length 0.  The packing is RFX_PACK_COUNT's
// (include/rufus_hip.h): A0 C1 G2 T3 in either case with the ACGT mask bit set, everything else code 0 and no mask bit.
//
// How a block is made of it (rfx_fasta.hip; the harness does the same serially):
//   line i = text[ls[i], ls[i + 1] - 1)             ls = the line starts; a last line without '\n' ends at n (ls = n + 1)
//   fa_line_key(line)                               header count in the high half, sequence bytes in the low half:
//                                                   ONE exclusive scan gives a line's record and its first base's index
//                                                   among all bases of the text (32 bits each: a text is < 4 GiB)
//   the NON-EMPTY sequence lines, compacted         ne_base[q] = first base index of line q, ne_src[q] = its first byte
//   fa_pack_word                                    one output code word: finds the line that holds its first base by
//                                                   binary search in ne_base and walks on from line to line
//
// Bounds.  Every text byte is read through fa_u8 at an index that has been compared with the text's byte count just
// before.  The arrays a function is handed are read at indices below the counts it is handed with them.  Nothing writes
// except through the two output pointers of fa_pack_word.
//
// Termination.  The binary searches halve a range of at most 2^32.  fa_pack_word's outer loop consumes at least one base
// per line step -- a line of the compacted list holds at least one, and a list that says otherwise ends the loop -- so it
// runs at most 32 line steps and 32 bases whatever the text and the lists hold.
#pragma once
#include <stdint.h>

#if defined(__HIP__)
#include <hip/hip_runtime.h>
#define RFX_FASTA_HD __host__ __device__ __forceinline__
#else
#define RFX_FASTA_HD inline
#endif

RFX_FASTA_HD uint32_t fa_u8(const uint8_t* t, uint64_t i) { return t[i]; }

// line [b, e) of text[0, n): e = where its '\n' lies, or n
RFX_FASTA_HD bool fa_is_header(const uint8_t* t, uint64_t n, uint64_t b, uint64_t e) { return b < e && b < n && fa_u8(t, b) == '>'; }
// header: 1 << 32; sequence line: its bytes
RFX_FASTA_HD uint64_t fa_line_key(const uint8_t* t, uint64_t n, uint64_t b, uint64_t e) {
  if (e < b) return 0;
  return fa_is_header(t, n, b, e) ? 1ull << 32 : e - b;
}
RFX_FASTA_HD uint32_t fa_key_headers(uint64_t key) { return (uint32_t)(key >> 32); }
RFX_FASTA_HD uint32_t fa_key_bases(uint64_t key) { return (uint32_t)key; }

// jf mer_dna.hpp:46-63 (rfx_host.cpp PackLut, RFX_PACK_COUNT): A/C/G/T in either case
RFX_FASTA_HD bool fa_is_acgt(uint32_t ch) {
  const uint32_t u = ch & 0xDFu;
  return u == 'A' || u == 'C' || u == 'G' || u == 'T';
}
RFX_FASTA_HD uint32_t fa_base_code(uint32_t ch) {  // of an A/C/G/T in either case: A0 C1 G2 T3
  const uint32_t x = (ch >> 1) & 3u;
  return x ^ (x >> 1);
}

// The last i in [0, n) with v[i] <= x; n >= 1 and v[0] <= x (else 0).
RFX_FASTA_HD uint32_t fa_last_le_u64(const uint64_t* v, uint32_t n, uint64_t x) {
  uint32_t lo = 0, hi = n;
  while (hi - lo > 1u) {
    const uint32_t mid = lo + (hi - lo) / 2u;
    if (v[mid] <= x) lo = mid;
    else hi = mid;
  }
  return lo;
}
RFX_FASTA_HD uint32_t fa_last_le_u32(const uint32_t* v, uint32_t n, uint32_t x) {
  uint32_t lo = 0, hi = n;
  while (hi - lo > 1u) {
    const uint32_t mid = lo + (hi - lo) / 2u;
    if (v[mid] <= x) lo = mid;
    else hi = mid;
  }
  return lo;
}

// Bases [gb, gb + nb) of the text's bases (nb <= 32; gb + nb <= ne_base[n_ne], the text's bases) as one code word and one
// mask word.  ne_base[0 .. n_ne] ascending, ne_base[n_ne] = all bases; ne_src[q] = the byte offset of line q's first base.
RFX_FASTA_HD void fa_pack_word(const uint8_t* t, uint64_t n, const uint32_t* ne_base, const uint32_t* ne_src, uint32_t n_ne,
                               uint32_t gb, uint32_t nb, uint64_t* code, uint32_t* mask) {
  uint64_t c = 0;
  uint32_t m = 0, b = 0;
  if (nb > 32u) nb = 32u;
  uint32_t q = n_ne ? fa_last_le_u32(ne_base, n_ne, gb) : 0u;
  while (b < nb && q < n_ne) {
    const uint32_t at = gb + b, lb = ne_base[q], le = ne_base[q + 1];
    if (at < lb || at >= le) break;  // (a line of the list holds at least this base: a list that says otherwise ends the word)
    const uint32_t take = le - at < nb - b ? le - at : nb - b;
    const uint64_t src = (uint64_t)ne_src[q] + (at - lb);
    for (uint32_t i = 0; i < take; ++i) {
      if (src + i >= n) break;
      const uint32_t ch = fa_u8(t, src + i);
      if (fa_is_acgt(ch)) {
        c |= (uint64_t)fa_base_code(ch) << (2u * (b + i));
        m |= 1u << (b + i);
      }
    }
    b += take;
    ++q;
  }
  *code = c;
  *mask = m;
}
