// A BAM record printed as `samtools view | PassThroughSamCheck.stranded` prints it (src/PassThroughSamCheck.stranded.cpp:
// 184-223; src/PassThroughSamCheck.stranded.se.cpp:172-201 is the same switch): what the host tails of `RUFUS.Filter --bam`
// (rfx_bam_pairs.hpp) and `RUFUS.Filter.single --bam` (rfx_bam_single.hpp) write for the few records the device gathered.
// The record layout is rfx_bam_core.h's; no device here.
#pragma once
#include <algorithm>
#include <string>

#include "../rfx_bam_core.h"
#include "rfx_sam.hpp"

namespace rfxsam {

// SEQ and QUAL of the record at byte p of b, which bam_valid accepts: "=ACMGRSVTWYHKDBN"[nibble] and 33 + min(q, 93), `*`
// for a record without bases or without qualities (qual[0] == 0xFF); flag & 16: reverse complement with every base
// other than A C G T N dropped, the quality string reversed whole.
[[maybe_unused]] void bam_print_stranded(const uint8_t* b, uint64_t p, std::string& seq, std::string& qual, std::string& tmp) {
  const uint32_t l_seq = (uint32_t)bam_l_seq(b, p);
  const uint64_t sq = bam_seq_offset(b, p), ql = sq + (l_seq + 1u) / 2u;
  seq.resize(l_seq);
  for (uint32_t i = 0; i < l_seq; ++i) seq[i] = "=ACMGRSVTWYHKDBN"[bam_nibble(b, sq, i)];
  if (l_seq == 0) seq = "*";
  if (l_seq == 0 || bam_u8(b, ql) == 0xFFu) {
    qual = "*";
  } else {
    qual.resize(l_seq);
    for (uint32_t i = 0; i < l_seq; ++i) qual[i] = (char)(33 + std::min<uint32_t>(bam_u8(b, ql + i), 93u));
  }
  if (bam_flag(b, p) & 16u) {
    revcomp_into(tmp, Field{seq.data(), seq.size()});
    seq.swap(tmp);
    reverse_into(tmp, Field{qual.data(), qual.size()});
    qual.swap(tmp);
  }
}

}  // namespace rfxsam
