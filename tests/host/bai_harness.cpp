// Host harness of tests/test_bai_host.py: rufus_amd/csrc/host/rfx_bai.hpp (region text, BAI reader, the one-range query)
// and the region test of rufus_amd/csrc/rfx_bam_core.h -- the statements k_bam_region runs -- built with
// -fsanitize=address,undefined.  Every buffer handed to the code under test is a heap block of exactly its length, so a
// read behind it is a report.
//
//   spec                                  the specification's values of reg2bin / reg2bins
//   region TEXT NAME...                   "ok tid beg end" or "refused <why>"
//   query BAI BAM_SIZE N_REF QUERIES      "refused <why>", or per line "tid beg end" of QUERIES "empty" / "start stop"
//   trunc BAI BAM_SIZE N_REF              read_index on every prefix: "trunc accepted <lengths...>"
//   recs FILE N_REF TID BEG END           FILE = whole records: per record "end_pos in_region"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../rufus_amd/csrc/host/rfx_bai.hpp"
#include "../../rufus_amd/csrc/rfx_bam_core.h"

static std::unique_ptr<uint8_t[]> slurp(const char* path, size_t* n) {
  FILE* f = fopen(path, "rb");
  if (!f) {
    fprintf(stderr, "cannot open %s\n", path);
    exit(2);
  }
  fseek(f, 0, SEEK_END);
  *n = (size_t)ftell(f);
  fseek(f, 0, SEEK_SET);
  std::unique_ptr<uint8_t[]> d(new uint8_t[*n ? *n : 1]);
  if (*n && fread(d.get(), 1, *n, f) != *n) exit(2);
  fclose(f);
  return d;
}

int main(int argc, char** argv) {
  const std::string cmd = argc > 1 ? argv[1] : "";
  if (cmd == "spec") {
    printf("reg2bin %u %u %u\n", rfxbai::reg2bin(0, 1 << 14), rfxbai::reg2bin(0, 1 << 29), rfxbai::reg2bin(1 << 14, (1 << 14) + 1));
    printf("reg2bins_one %zu\n", rfxbai::reg2bins(123456, 123457).size());
    printf("reg2bins_all %zu\n", rfxbai::reg2bins(0, 1ll << 29).size());
    printf("reg2bins_none %zu %zu\n", rfxbai::reg2bins(5, 5).size(), rfxbai::reg2bins(1ll << 29, 1ll << 30).size());
    return 0;
  }
  if (cmd == "region" && argc >= 3) {
    std::vector<std::string> names(argv + 3, argv + argc);
    rfxbai::Region r;
    std::string why;
    if (rfxbai::parse_region(argv[2], names, &r, &why)) printf("ok %d %lld %lld\n", (int)r.tid, (long long)r.beg, (long long)r.end);
    else printf("refused %s\n", why.c_str());
    return 0;
  }
  if (cmd == "query" && argc == 6) {
    size_t n = 0;
    auto d = slurp(argv[2], &n);
    std::unique_ptr<uint8_t[]> exact(new uint8_t[n ? n : 1]);
    memcpy(exact.get(), d.get(), n);
    rfxbai::Index ix;
    std::string why;
    if (!rfxbai::read_index(exact.get(), n, atoi(argv[4]), strtoull(argv[3], nullptr, 10), &ix, &why)) {
      printf("refused %s\n", why.c_str());
      return 0;
    }
    FILE* q = fopen(argv[5], "r");
    if (!q) return 2;
    int tid;
    long long beg, end;
    while (fscanf(q, "%d %lld %lld", &tid, &beg, &end) == 3) {
      const rfxbai::Range r = rfxbai::query(ix, tid, beg, end);
      if (r.empty) printf("empty\n");
      else printf("%llu %llu\n", (unsigned long long)r.start, (unsigned long long)r.stop);
    }
    fclose(q);
    return 0;
  }
  if (cmd == "trunc" && argc == 5) {
    size_t n = 0;
    auto d = slurp(argv[2], &n);
    printf("trunc accepted");
    for (size_t len = 0; len <= n; ++len) {
      std::unique_ptr<uint8_t[]> exact(new uint8_t[len ? len : 1]);
      memcpy(exact.get(), d.get(), len);
      rfxbai::Index ix;
      std::string why;
      if (rfxbai::read_index(exact.get(), len, atoi(argv[4]), strtoull(argv[3], nullptr, 10), &ix, &why)) printf(" %zu", len);
    }
    printf("\n");
    return 0;
  }
  if (cmd == "recs" && argc == 7) {
    size_t n = 0;
    auto d = slurp(argv[2], &n);
    const int32_t n_ref = atoi(argv[3]), tid = atoi(argv[4]);
    const int64_t beg = atoll(argv[5]), end = atoll(argv[6]);
    uint64_t p = 0;
    while (p < n) {
      const uint64_t nx = bam_next(d.get(), p, n);
      if (nx == BAM_STOP || bam_valid(d.get(), p, n_ref) != BAM_OK) {
        fprintf(stderr, "not a record at byte %llu\n", (unsigned long long)p);
        return 3;
      }
      // the record alone in a block of its own length: a read behind it is a report
      std::unique_ptr<uint8_t[]> one(new uint8_t[nx - p]);
      memcpy(one.get(), d.get() + p, nx - p);
      printf("%lld %d\n", (long long)bam_end_pos(one.get(), 0), (int)bam_in_region(one.get(), 0, tid, beg, end));
      p = nx;
    }
    return 0;
  }
  fprintf(stderr, "usage: bai_harness spec | region | query | trunc | recs\n");
  return 2;
}
