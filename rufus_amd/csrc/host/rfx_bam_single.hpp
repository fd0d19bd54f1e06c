// The host tail of `RUFUS.Filter.single --bam` (rfx_ingest.hpp BamSingleFilter): the records rfx_bam_gather_hits pulled out
// of an arena -- every kept record whose hit count reaches the threshold, with that count -- printed as
// `samtools view | PassThroughSamCheck.stranded.se | RUFUS.Filter.single` writes them: the stranded printer's SEQ and QUAL
// (rfx_bam_print.hpp; src/PassThroughSamCheck.stranded.se.cpp:172-201) under `@QNAME:MH<hits>`
// (src/RUFUS.Filter.ss.cpp:194-203).  Nothing is paired and nothing waits: a record is printed and forgotten.
// A reverse-strand `*` prints as an empty sequence line: a kept record of 0 windows, written only when the threshold is
// <= 0.  No device here: tests/host/filter_single_harness.cpp runs this file as it is.
#pragma once
#include <cstdio>
#include <string>

#include "../rfx_bam_core.h"
#include "rfx_bam_print.hpp"

namespace rfxsam {

struct BamSingleTail {
  std::string out;  // the FASTQ text of what add() has been given since the caller last cleared it
  std::string seq, qual, tmp;
  uint64_t records = 0, windows = 0;  // over the whole run: the printed records, the sum of their hit counts

  // b[0, bytes): n gathered records one behind the other, block_size field and all; hits[j]: the count of the j-th.
  // Every record is checked before anything of it is read -- whole inside the bytes, bam_valid -- and the records must
  // add up to `bytes` exactly.  false with *why set: refused; `out` then holds the records in front of the bad one.
  bool add(const uint8_t* b, uint64_t bytes, const uint32_t* hits, uint64_t n, std::string* why) {
    uint64_t p = 0;
    char num[16];
    for (uint64_t j = 0; j < n; ++j) {
      if (p + BAM_FIXED > bytes || bam_next(b, p, bytes) == BAM_STOP) {
        *why = "gathered record " + std::to_string(j) + " is cut by the end of the gathered bytes";
        return false;
      }
      if (bam_valid(b, p, 0x7FFFFFFF) != BAM_OK) {
        *why = "gathered record " + std::to_string(j) + " is not a BAM record";
        return false;
      }
      bam_print_stranded(b, p, seq, qual, tmp);
      out.push_back('@');
      out.append((const char*)b + p + BAM_FIXED, bam_name_len(b, p));
      out.append(":MH");
      const int digits = snprintf(num, sizeof num, "%u", hits[j]);
      out.append(num, (size_t)digits);
      out.push_back('\n');
      out += seq;
      out.append("\n+\n");
      out += qual;
      out.push_back('\n');
      ++records;
      windows += hits[j];
      p = bam_next(b, p, bytes);
    }
    if (p != bytes) {
      *why = "the gathered records do not add up to the gathered bytes";
      return false;
    }
    return true;
  }
};

}  // namespace rfxsam
