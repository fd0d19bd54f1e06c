// Host-only harness for `RUFUS.Filter --bam`: the RFX_BAM_HD functions the kernels of rufus_amd/csrc/rfx_bam.hip run for the
// stranded filter form and the name hash (rfx_bam_core.h: bam_filter_len, bam_filter_word, bam_name_hash) and the host tail
// of the route (rufus_amd/csrc/host/rfx_bam_pairs.hpp: the stranded printer and the pairing walk), as they are, under
// AddressSanitizer and UBSan.  No kernel is copied here: the record chain is walked serially with bam_next.
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined filter_bam_harness.cpp
//   harness pack  DATA first n_ref exclude min_q OUT   -> OUT.len (u32) OUT.codes (u64) OUT.good (u32) OUT.hash (u64)
//   harness pairs DATA first n_ref exclude FLAGS OUT   -> OUT.m1 OUT.m2; FLAGS: a byte per kept record, bit 0 = hit, bit 1 =
//                                                        the record is in the subset the walk is given
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iterator>
#include <vector>

#include "../../rufus_amd/csrc/host/rfx_bam_pairs.hpp"

static std::vector<uint8_t> slurp(const char* path) {
  std::ifstream f(path, std::ios::binary);
  if (!f.is_open()) {
    fprintf(stderr, "cannot open %s\n", path);
    exit(2);
  }
  return std::vector<uint8_t>(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
}
template <class T>
static void dump(const std::string& path, const std::vector<T>& v) {
  std::ofstream f(path, std::ios::binary);
  f.write((const char*)v.data(), (std::streamsize)(v.size() * sizeof(T)));
}

int main(int argc, char** argv) {
  if (argc != 8) {
    fprintf(stderr, "usage: see the head of the source\n");
    return 2;
  }
  const std::string mode = argv[1], out = argv[7];
  // (an exact-size heap copy: a read one byte behind the data is a sanitizer report)
  const std::vector<uint8_t> file = slurp(argv[2]);
  uint8_t* b = (uint8_t*)malloc(file.size() ? file.size() : 1);
  memcpy(b, file.data(), file.size());
  const uint64_t end = file.size(), first = strtoull(argv[3], nullptr, 0);
  const int32_t n_ref = atoi(argv[4]);
  const uint32_t exclude = (uint32_t)strtoul(argv[5], nullptr, 0);
  std::vector<uint64_t> kept;
  uint64_t n_rec = 0;
  for (uint64_t p = first; p < end;) {
    const uint64_t nx = bam_next(b, p, end);
    if (nx == BAM_STOP || bam_valid(b, p, n_ref) != BAM_OK) {
      fprintf(stderr, "no valid record at byte %llu\n", (unsigned long long)p);
      return 1;
    }
    if (!(bam_flag(b, p) & exclude)) kept.push_back(p);
    ++n_rec;
    p = nx;
  }
  if (mode == "pack") {
    const int min_q = atoi(argv[6]);
    std::vector<uint32_t> len, good;
    std::vector<uint64_t> codes, hash;
    for (uint64_t p : kept) {
      const uint32_t L = bam_filter_len(b, p);
      len.push_back(L);
      hash.push_back(bam_name_hash(b, p));
      for (uint32_t j = 0; j < (L + 31) / 32; ++j) {
        uint64_t c;
        uint32_t g;
        bam_filter_word(b, p, j, L, min_q, &c, &g);
        codes.push_back(c);
        good.push_back(g);
      }
    }
    dump(out + ".len", len);
    dump(out + ".codes", codes);
    dump(out + ".good", good);
    dump(out + ".hash", hash);
    printf("ok records %llu kept %zu words %zu\n", (unsigned long long)n_rec, kept.size(), codes.size());
  } else if (mode == "pairs") {
    const std::vector<uint8_t> flags = slurp(argv[6]);
    if (flags.size() != kept.size()) {
      fprintf(stderr, "%zu flags for %zu kept records\n", flags.size(), kept.size());
      return 1;
    }
    rfxsam::BamPairTail tail;
    for (size_t i = 0; i < kept.size(); ++i)
      if (flags[i] & 2) tail.add(b, kept[i], flags[i] & 1);
    std::ofstream(out + ".m1", std::ios::binary).write(tail.walk.o1.data(), (std::streamsize)tail.walk.o1.size());
    std::ofstream(out + ".m2", std::ios::binary).write(tail.walk.o2.data(), (std::streamsize)tail.walk.o2.size());
    printf("ok records %llu kept %zu walked %llu pairs %llu pulled %llu\n", (unsigned long long)n_rec, kept.size(),
           (unsigned long long)tail.records, tail.walk.n_pairs, tail.walk.n_found);
  } else {
    return 2;
  }
  free(b);
  return 0;
}
