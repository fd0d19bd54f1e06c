// `samtools view X.bam CHR:BEG-END` in front of the two BAM feeders (runRufus.sh -R: :599, :639, :964-967): the region's
// text, the BAM index (section 5.2 of the SAM specification) and the ONE file range a region needs.  Pure host code, no
// device: tests/host/bai_harness.cpp runs every statement here under AddressSanitizer and UBSan.
//
// The index only says where to look.  Whether a record is in the region is decided per record on the device
// (rfx_bam_core.h bam_in_region), so any SUPERSET of the region's records gives the exact result: one range from the
// lowest chunk start to the highest chunk end is enough, and no result depends on how fine the index is.
//
// Bounds.  read_index reads through Cursor, which refuses a read that does not lie inside [0, n); counts are checked
// against the bytes that are left BEFORE anything is reserved, so a hostile count costs no memory.  Nothing here writes
// outside its own vectors.
#pragma once
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

namespace rfxbai {

constexpr int64_t MAX_POS = 1ll << 29;  // what a BAI's binning scheme covers; a region without END ends here
constexpr uint32_t META_BIN = 37450;    // the pseudo-bin: two "chunks" of metadata, no file offsets

// ---- the binning scheme (section 5.3) ---------------------------------------------------------------------------------
inline uint32_t reg2bin(int64_t beg, int64_t end) {
  --end;
  if (beg >> 14 == end >> 14) return (uint32_t)(((1 << 15) - 1) / 7 + (beg >> 14));
  if (beg >> 17 == end >> 17) return (uint32_t)(((1 << 12) - 1) / 7 + (beg >> 17));
  if (beg >> 20 == end >> 20) return (uint32_t)(((1 << 9) - 1) / 7 + (beg >> 20));
  if (beg >> 23 == end >> 23) return (uint32_t)(((1 << 6) - 1) / 7 + (beg >> 23));
  if (beg >> 26 == end >> 26) return (uint32_t)(((1 << 3) - 1) / 7 + (beg >> 26));
  return 0;
}
// the bins that may hold a record overlapping [beg, end), 0 <= beg < end <= 2^29, ascending
inline std::vector<uint32_t> reg2bins(int64_t beg, int64_t end) {
  std::vector<uint32_t> bins;
  if (beg < 0) beg = 0;
  if (end > MAX_POS) end = MAX_POS;
  if (beg >= end) return bins;
  --end;
  bins.push_back(0);
  for (int64_t k = 1 + (beg >> 26); k <= 1 + (end >> 26); ++k) bins.push_back((uint32_t)k);
  for (int64_t k = 9 + (beg >> 23); k <= 9 + (end >> 23); ++k) bins.push_back((uint32_t)k);
  for (int64_t k = 73 + (beg >> 20); k <= 73 + (end >> 20); ++k) bins.push_back((uint32_t)k);
  for (int64_t k = 585 + (beg >> 17); k <= 585 + (end >> 17); ++k) bins.push_back((uint32_t)k);
  for (int64_t k = 4681 + (beg >> 14); k <= 4681 + (end >> 14); ++k) bins.push_back((uint32_t)k);
  return bins;
}

// ---- the region's text ------------------------------------------------------------------------------------------------
// A text that is a reference's name as a whole is that whole reference, even if it holds a colon.  Otherwise it is cut
// at its LAST colon: NAME:BEG or NAME:BEG-END, 1-based and inclusive, commas in the numbers dropped -> [BEG - 1, END).
struct Region {
  int32_t tid = -1;
  int64_t beg = 0, end = MAX_POS;
};

// digits (commas dropped) from s[at]; at least one digit, at most 18 (no overflow); false otherwise
inline bool region_number(const std::string& s, size_t& at, int64_t* out) {
  int64_t v = 0;
  int digits = 0;
  for (; at < s.size() && ((s[at] >= '0' && s[at] <= '9') || s[at] == ','); ++at) {
    if (s[at] == ',') continue;
    if (++digits > 18) return false;
    v = v * 10 + (s[at] - '0');
  }
  *out = v;
  return digits > 0;
}

inline bool parse_region(const std::string& text, const std::vector<std::string>& names, Region* out, std::string* why) {
  auto find = [&](const std::string& name) {
    for (size_t i = 0; i < names.size(); ++i)
      if (names[i] == name) return (int32_t)i;
    return (int32_t)-1;
  };
  auto refuse = [&](const char* what) {
    *why = "region '" + text + "': " + what;
    return false;
  };
  *out = Region();
  if (text.empty()) return refuse("empty");
  out->tid = find(text);
  if (out->tid >= 0) return true;
  const size_t colon = text.rfind(':');
  if (colon == std::string::npos) return refuse("no reference of the BAM has this name");
  out->tid = find(text.substr(0, colon));
  if (out->tid < 0) return refuse("no reference of the BAM has this name");
  size_t at = colon + 1;
  int64_t beg = 0, end = MAX_POS;
  if (!region_number(text, at, &beg)) return refuse("BEG is not a number");
  if (beg < 1) return refuse("BEG is below 1 (coordinates are 1-based)");
  if (at < text.size() && text[at] == '-') {
    ++at;
    if (!region_number(text, at, &end)) return refuse("END is not a number");
    if (end < beg) return refuse("END lies in front of BEG");
  }
  if (at != text.size()) return refuse("trailing characters behind the coordinates");
  out->beg = beg - 1;
  out->end = end;
  return true;
}

// ---- the index --------------------------------------------------------------------------------------------------------
struct Chunk {
  uint32_t bin;
  uint64_t beg, end;  // virtual offsets: compressed offset of a block << 16 | offset inside its inflated data
};
struct Ref {
  std::vector<Chunk> chunks;      // of every bin but the pseudo-bin, in file order
  std::vector<uint64_t> ioffset;  // the linear index: a virtual offset per 16 kbp window
};
struct Index {
  std::vector<Ref> refs;
};

struct Cursor {
  const uint8_t* d;
  size_t n, at = 0;
  bool ok = true;
  size_t left() const { return n - at; }
  uint64_t get(unsigned bytes) {  // little endian; a read that does not fit: ok = false, 0
    if (!ok || left() < bytes) {
      ok = false;
      return 0;
    }
    uint64_t v = 0;
    for (unsigned i = 0; i < bytes; ++i) v |= (uint64_t)d[at + i] << (8 * i);
    at += bytes;
    return v;
  }
  int32_t i32() { return (int32_t)(uint32_t)get(4); }
  uint32_t u32() { return (uint32_t)get(4); }
  uint64_t u64() { return get(8); }
};

// d[0, n) = the index file's bytes.  n_ref: the BAM header's; bam_size: the BAM file's bytes.  false: *why says what is
// wrong, *out is unspecified.
inline bool read_index(const uint8_t* d, size_t n, int32_t n_ref, uint64_t bam_size, Index* out, std::string* why) {
  auto refuse = [&](const char* what) {
    *why = what;
    return false;
  };
  Cursor c{d, n};
  out->refs.clear();
  if (n < 8 || memcmp(d, "BAI\1", 4) != 0) return refuse("no BAI magic");
  c.at = 4;
  const int32_t refs = c.i32();
  if (refs != n_ref) return refuse("n_ref differs from the BAM header's");
  if ((uint64_t)refs > c.left() / 8) return refuse("truncated");  // (a reference takes at least n_bin and n_intv)
  out->refs.resize((size_t)refs);
  for (Ref& r : out->refs) {
    const int32_t n_bin = c.i32();
    if (!c.ok) return refuse("truncated");
    if (n_bin < 0) return refuse("negative n_bin");
    for (int32_t b = 0; b < n_bin; ++b) {
      const uint32_t bin = c.u32();
      const int32_t n_chunk = c.i32();
      if (!c.ok) return refuse("truncated");
      if (n_chunk < 0) return refuse("negative n_chunk");
      if ((uint64_t)n_chunk > c.left() / 16) return refuse("truncated");
      if (bin == META_BIN) {
        c.at += (size_t)n_chunk * 16;
        continue;
      }
      for (int32_t k = 0; k < n_chunk; ++k) {
        const uint64_t beg = c.u64(), end = c.u64();
        if (beg >= end) return refuse("a chunk that does not end behind its start");
        if ((beg >> 16) >= bam_size || (end >> 16) >= bam_size) return refuse("a chunk beyond the BAM file");
        r.chunks.push_back(Chunk{bin, beg, end});
      }
    }
    const int32_t n_intv = c.i32();
    if (!c.ok) return refuse("truncated");
    if (n_intv < 0) return refuse("negative n_intv");
    if ((uint64_t)n_intv > c.left() / 8) return refuse("truncated");
    r.ioffset.resize((size_t)n_intv);
    for (uint64_t& v : r.ioffset) {
      v = c.u64();
      if ((v >> 16) >= bam_size) return refuse("a linear index entry beyond the BAM file");
    }
  }
  if (c.left() != 0 && c.left() != 8) return refuse("bytes behind the last reference that are no n_no_coor");
  return true;
}

// ---- the query --------------------------------------------------------------------------------------------------------
struct Range {
  bool empty = true;
  uint64_t start = 0, stop = 0;  // virtual offsets: every record of the region starts in [start, stop)
};
inline Range query(const Index& ix, int32_t tid, int64_t beg, int64_t end) {
  Range out;
  if (tid < 0 || (size_t)tid >= ix.refs.size()) return out;
  if (beg < 0) beg = 0;
  const std::vector<uint32_t> bins = reg2bins(beg, end);  // ascending (empty: beg >= min(end, 2^29))
  if (bins.empty()) return out;
  const Ref& r = ix.refs[(size_t)tid];
  const uint64_t min_off = r.ioffset.empty() ? 0 : r.ioffset[std::min<size_t>((size_t)(beg >> 14), r.ioffset.size() - 1)];
  for (const Chunk& ch : r.chunks) {
    if (ch.end <= min_off || !std::binary_search(bins.begin(), bins.end(), ch.bin)) continue;
    const uint64_t from = std::max(ch.beg, min_off);
    if (out.empty || from < out.start) out.start = from;
    if (out.empty || ch.end > out.stop) out.stop = ch.end;
    out.empty = false;
  }
  return out;
}

}  // namespace rfxbai
