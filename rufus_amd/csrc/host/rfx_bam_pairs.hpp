// The host tail of `RUFUS.Filter --bam` (rfx_ingest.hpp BamPairFilter): the few BAM records the device gathered -- every
// record of every name with a hit -- printed as `samtools view | PassThroughSamCheck.stranded` prints them
// (src/PassThroughSamCheck.stranded.cpp:184-223: rfx_bam_print.hpp) and handed to the pairing walk `--sam` runs (rfx_sam.hpp
// PairWalk).
// The record layout is rfx_bam_core.h's; no device here: tests/host/filter_bam_harness.cpp runs this file as it is.
#pragma once
#include <deque>
#include <string>

#include "../rfx_bam_core.h"
#include "rfx_bam_print.hpp"
#include "rfx_sam.hpp"

namespace rfxsam {

// The walk over the gathered records, in stream order.  A record's bytes stay in `kept` for the whole walk: the subset is
// small (the hit names' records), and a waiting record is a pointer, as in the text route.
struct BamPairTail {
  PairWalk walk;
  std::deque<std::string> kept;  // name, sequence, quality of a record, one behind the other
  std::deque<Rec> recs;
  std::string seq, qual, tmp;
  uint64_t records = 0;
  // the record at byte p of b (whole: block_size and all); hit: its bit from the scan
  void add(const uint8_t* b, uint64_t p, bool hit) {
    bam_print_stranded(b, p, seq, qual, tmp);
    const uint32_t nn = bam_name_len(b, p);
    kept.emplace_back();
    std::string& s = kept.back();
    s.reserve(nn + seq.size() + qual.size());
    s.assign((const char*)b + p + BAM_FIXED, nn);
    s += seq;
    s += qual;
    Rec r;
    r.name = s.data();
    r.name_len = nn;
    r.seq = s.data() + nn;
    r.seq_len = (uint32_t)seq.size();
    r.qual = s.data() + nn + seq.size();
    r.qual_len = (uint32_t)qual.size();
    r.hash = name_hash(r.name, r.name_len);
    recs.push_back(r);
    ++records;
    (void)walk.meet(recs.back(), hit ? 1u : 0u);  // (a deque's elements stay where they are: a waiting record is safe)
  }
};

}  // namespace rfxsam
