// Stand-alone host harness of the BGZF decoder core (rufus_amd/csrc/rfx_bgzf_core.h): the statements the kernel
// k_bgzf_inflate runs, here with a serial copy as the output policy, built with -fsanitize=address,undefined by
// tests/test_bgzf_host.py.  Every payload and every output buffer is a heap block of exactly its size, so a read or write
// one byte outside is a sanitizer report.
//
//   bgzf_harness FILE...     each FILE: a sequence of BGZF blocks
//
// Per file it prints
//   file <name>
//   block <i> status <code> isize <n>          (one per block; status 0 = decoded, CRC and ISIZE match)
//   format <offset>                            (the bytes at <offset> are no BGZF block header: the walk ends there)
//   crc <8 hex digits> bytes <n>               (CRC-32 and size of the concatenated output of the blocks with status 0)
//   types stored=<n> fixed=<n> dynamic=<n>     (deflate blocks by type)
//   deflate_blocks_max <n>                     (most deflate blocks in one BGZF block)
//   longest_code <bits>
//   dist <smallest> <largest>                  (0 0: no match)
//   len <smallest> <largest>
//   cl_cross <0|1>                             (a code-length run crossed from the literal/length into the distance lengths)
//   one_dist_code <0|1>                        (a distance table had one code)
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

struct Stats {
  uint64_t types[4] = {0, 0, 0, 0};
  uint32_t in_this = 0, blocks_max = 0, longest = 0, dmin = 0, dmax = 0, lmin = 0, lmax = 0;
  bool cross = false, one_dist = false;
  void block(uint32_t type) {
    ++types[type & 3];
    if (++in_this > blocks_max) blocks_max = in_this;
  }
  void code_len(uint32_t mx) {
    if (mx > longest) longest = mx;
  }
  void cl_run(uint32_t, uint32_t idx, uint32_t rep, uint32_t nlit) {
    if (idx < nlit && idx + rep > nlit) cross = true;
  }
  void dist_codes(const uint16_t* count, uint32_t mx) {
    uint32_t n = 0;
    for (uint32_t l = 1; l <= mx && l < 16; ++l) n += count[l];
    if (n == 1) one_dist = true;
  }
  void match(uint32_t len, uint32_t d) {
    if (!dmin || d < dmin) dmin = d;
    if (d > dmax) dmax = d;
    if (!lmin || len < lmin) lmin = len;
    if (len > lmax) lmax = len;
  }
};
static Stats g_stats;
#define RFX_BGZF_STAT(x) g_stats.x
#include "../../rufus_amd/csrc/rfx_bgzf_core.h"

struct SerialOut {  // the kernel's formulas, one byte at a time
  uint8_t* out;
  void literal(uint32_t pos, uint32_t byte) { out[pos] = (uint8_t)byte; }
  void match(uint32_t pos, uint32_t len, uint32_t dist) {
    for (uint32_t i = 0; i < len; ++i) out[pos + i] = out[pos - dist + i % dist];
  }
  void stored(uint32_t pos, const uint8_t* src, uint32_t n) {
    for (uint32_t i = 0; i < n; ++i) out[pos + i] = src[i];
  }
  void end() {}
};

static int run_file(const char* path) {
  FILE* f = fopen(path, "rb");
  if (!f) {
    fprintf(stderr, "cannot open %s\n", path);
    return 2;
  }
  std::vector<uint8_t> data;
  uint8_t chunk[1 << 16];
  size_t got;
  while ((got = fread(chunk, 1, sizeof chunk, f)) > 0) data.insert(data.end(), chunk, chunk + got);
  fclose(f);
  printf("file %s\n", path);
  g_stats = Stats();
  bgzf_tables* tables = new bgzf_tables();
  uint32_t reg = 0xFFFFFFFFu;
  uint64_t total = 0, at = 0;
  for (uint32_t i = 0; at < data.size(); ++i) {
    uint32_t bsize = 0, pay_off = 0, pay_len = 0, isize = 0, crc = 0;
    const int h = bgzf_block_header(data.data() + at, data.size() - at, &bsize, &pay_off, &pay_len, &isize, &crc);
    if (h != 0) {
      printf("format %llu\n", (unsigned long long)at);
      break;
    }
    uint8_t* in = (uint8_t*)malloc(pay_len ? pay_len : 1);
    uint8_t* out = (uint8_t*)malloc(isize ? isize : 1);
    memcpy(in, data.data() + at + pay_off, pay_len);
    g_stats.in_this = 0;
    SerialOut so{out};
    uint32_t st = bgzf_inflate(in, in + pay_len, isize, *tables, so);
    if (st == BGZF_OK) {
      uint32_t x = 0;
      for (uint32_t lane = 0; lane < 64; ++lane) x ^= bgzf_crc_lane(out, isize, lane);
      if (x != bgzf_crc_update(0xFFFFFFFFu, out, isize)) {
        fprintf(stderr, "the lanes' CRC is not the serial CRC\n");
        return 3;
      }
      if (~x != crc) st = BGZF_E_CRC;
    }
    printf("block %u status %u isize %u\n", i, st, isize);
    if (st == BGZF_OK) {
      reg = bgzf_crc_update(reg, out, isize);
      total += isize;
    }
    free(in);
    free(out);
    at += bsize;
  }
  delete tables;
  printf("crc %08x bytes %llu\n", ~reg, (unsigned long long)total);
  printf("types stored=%llu fixed=%llu dynamic=%llu\n", (unsigned long long)g_stats.types[0], (unsigned long long)g_stats.types[1],
         (unsigned long long)g_stats.types[2]);
  printf("deflate_blocks_max %u\nlongest_code %u\ndist %u %u\nlen %u %u\ncl_cross %d\none_dist_code %d\n", g_stats.blocks_max,
         g_stats.longest, g_stats.dmin, g_stats.dmax, g_stats.lmin, g_stats.lmax, (int)g_stats.cross, (int)g_stats.one_dist);
  return 0;
}

int main(int argc, char** argv) {
  if (argc < 2) {
    fprintf(stderr, "usage: bgzf_harness FILE...\n");
    return 2;
  }
  for (int i = 1; i < argc; ++i) {
    const int rc = run_file(argv[i]);
    if (rc) return rc;
  }
  return 0;
}
