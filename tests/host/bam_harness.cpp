// Stand-alone host harness of the BAM record core (rufus_amd/csrc/rfx_bam_core.h): guess / walk / repair / starts -- the
// statements the kernels of rfx_bam.hip run -- written serially, built with -fsanitize=address,undefined by
// tests/test_bam_host.py.  Every input is a heap block of exactly its size, so a read one byte outside is a sanitizer
// report.  Every run is also compared with the naive walk (one bam_next after the other from `skip`).
//
//   bam_harness run FILE N_REF SKIP TILE NO_GUESS STARTS_OUT    the record starts (u32 each) go to STARTS_OUT
//   bam_harness trunc FILE N_REF SKIP TILE                      every prefix of FILE, with and without guesses
//   bam_harness flips FILE N_REF SKIP TILE SEED COUNT           COUNT seeded single-byte flips, with and without guesses
//   bam_harness pack                                            bam_pack_word against a table lookup, every nibble pair
// Output: one line per run
//   status <bam_status of the lowest failing chain record> bad_at <its offset> records <n> cut <c> changed <g> rounds <r>
// and at the end
//   refusals <count per bam_status 1 .. 5>
//   wrong_guess <runs in which repair changed a guess>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

struct Stats {
  unsigned long long refusals[8] = {0};
  unsigned long long wrong_guess = 0;
  void refusal(uint32_t s) { refusals[s & 7]++; }
} g_stats;
#define RFX_BAM_STAT(x) g_stats.x
#include "../../rufus_amd/csrc/rfx_bam_core.h"

constexpr uint32_t NONE = 0xFFFFFFFFu;

struct Result {
  uint32_t status = 0, bad_at = NONE, changed = 0, rounds = 0;
  uint64_t cut = 0;
  std::vector<uint32_t> starts;
};

struct StartVisit {
  const uint8_t* b;
  int32_t n_ref;
  Result* r;
  void operator()(uint64_t p, uint32_t) {
    r->starts.push_back((uint32_t)p);
    const uint32_t st = bam_valid(b, p, n_ref);
    if (st != BAM_OK && (uint32_t)p < r->bad_at) {
      r->bad_at = (uint32_t)p;
      r->status = st;
    }
  }
};

static Result tiled(const uint8_t* b, uint64_t n, uint64_t skip, int32_t n_ref, uint32_t T, bool no_guess) {
  Result res;
  res.cut = skip;
  if (n == 0) return res;
  const uint32_t n_tiles = (uint32_t)((n + T - 1) / T);
  std::vector<uint32_t> in(n_tiles, NONE), guess(n_tiles, NONE), ex[2] = {std::vector<uint32_t>(n_tiles), std::vector<uint32_t>(n_tiles)};
  std::vector<uint64_t> cnt(n_tiles + 1, 0);
  auto limit = [&](uint32_t t) { return ((uint64_t)t + 1) * T < n ? ((uint64_t)t + 1) * T : n; };
  for (uint32_t t = 0; t < n_tiles; ++t) {  // k_bam_guess
    uint32_t g = NONE;
    if (t == 0) g = (uint32_t)skip;
    else if (!no_guess)
      for (uint64_t c = (uint64_t)t * T; c < limit(t); ++c)
        if (bam_guess_ok(b, c, n, n_ref)) {
          g = (uint32_t)c;
          break;
        }
    in[t] = guess[t] = g;
  }
  bam_no_visit nv;
  for (uint32_t t = 0; t < n_tiles; ++t) {  // k_bam_walk
    uint32_t c = 0;
    ex[0][t] = (uint32_t)bam_walk(b, in[t], limit(t), n, &c, nv);
    cnt[t] = c;
  }
  int cur = 0;
  for (;;) {  // k_bam_repair, one round per turn
    uint32_t changed = 0;
    for (uint32_t t = 0; t < n_tiles; ++t) {
      if (t == 0 || in[t] == ex[cur][t - 1]) {
        ex[cur ^ 1][t] = ex[cur][t];
        continue;
      }
      in[t] = ex[cur][t - 1];
      uint32_t c = 0;
      ex[cur ^ 1][t] = (uint32_t)bam_walk(b, in[t], limit(t), n, &c, nv);
      cnt[t] = c;
      ++changed;
    }
    cur ^= 1;
    if (!changed) break;
    if (++res.rounds > n_tiles) {
      fprintf(stderr, "the chain did not settle in %u rounds\n", n_tiles);
      exit(3);
    }
  }
  StartVisit sv{b, n_ref, &res};
  for (uint32_t t = 0; t < n_tiles; ++t) {  // k_bam_starts
    uint32_t c = 0;
    const uint64_t e = bam_walk(b, in[t], limit(t), n, &c, sv);
    if (c != cnt[t]) {
      fprintf(stderr, "tile %u: %u records now, %llu before\n", t, c, (unsigned long long)cnt[t]);
      exit(3);
    }
    if (t == n_tiles - 1) res.cut = e;
    if (guess[t] != in[t]) ++res.changed;
  }
  if (res.changed) g_stats.wrong_guess++;
  return res;
}

static void naive_check(const uint8_t* b, uint64_t n, uint64_t skip, const Result& r, const char* what) {
  std::vector<uint32_t> starts;
  uint64_t p = skip, steps = 0;
  for (uint64_t nx; (nx = bam_next(b, p, n)) != BAM_STOP; p = nx) {
    starts.push_back((uint32_t)p);
    if (nx < p + 4 || ++steps > n / 4 + 1) {
      fprintf(stderr, "%s: a walk that does not advance\n", what);
      exit(3);
    }
  }
  if (starts != r.starts || p != r.cut) {
    fprintf(stderr, "%s: the tiled chain differs from the naive walk (%zu / %zu records, cut %llu / %llu)\n", what, r.starts.size(),
            starts.size(), (unsigned long long)r.cut, (unsigned long long)p);
    exit(3);
  }
}

static void report(const Result& r) {
  printf("status %u bad_at %u records %zu cut %llu changed %u rounds %u\n", r.status, r.bad_at, r.starts.size(),
         (unsigned long long)r.cut, r.changed, r.rounds);
}

static uint8_t* exact_copy(const std::vector<uint8_t>& v, size_t n) {  // a heap block of exactly n bytes
  uint8_t* p = (uint8_t*)malloc(n ? n : 1);
  if (n) memcpy(p, v.data(), n);
  return p;
}

int main(int argc, char** argv) {
  if (argc >= 2 && !strcmp(argv[1], "pack")) {
    static const char letters[] = "=ACMGRSVTWYHKDBN";
    unsigned long long checked = 0;
    for (uint32_t nb = 0; nb <= 32; ++nb)
      for (uint32_t seed = 0; seed < 4096; ++seed) {
        uint32_t w[4], x = seed * 2654435761u + nb;
        for (int i = 0; i < 4; ++i) w[i] = x = x * 1664525u + 1013904223u;
        if (seed < 256) w[0] = seed | seed << 8 | seed << 16 | seed << 24;  // every nibble pair in every byte
        uint64_t c = 0, want_c = 0;
        uint32_t m = 0, want_m = 0;
        bam_pack_word(w, nb, &c, &m);
        for (uint32_t i = 0; i < nb; ++i) {
          const uint8_t byte = ((const uint8_t*)w)[i >> 1];  // (little endian: stream order)
          const char ch = letters[(i & 1) ? byte & 15 : byte >> 4];
          const char* at = strchr("ACGT", ch);
          if (at) {
            want_c |= (uint64_t)(at - "ACGT") << (2 * i);
            want_m |= 1u << i;
          }
        }
        if (c != want_c || m != want_m) {
          fprintf(stderr, "bam_pack_word differs at nb %u seed %u\n", nb, seed);
          return 3;
        }
        ++checked;
      }
    printf("pack ok %llu\n", checked);
    return 0;
  }
  if (argc < 6) return 2;
  FILE* f = fopen(argv[2], "rb");
  if (!f) return 2;
  std::vector<uint8_t> file;
  uint8_t tmp[65536];
  for (size_t k; (k = fread(tmp, 1, sizeof tmp, f)) > 0;) file.insert(file.end(), tmp, tmp + k);
  fclose(f);
  const int32_t n_ref = atoi(argv[3]);
  const uint64_t skip = strtoull(argv[4], nullptr, 10);
  const uint32_t T = (uint32_t)atoi(argv[5]);
  if (T < 256 || (T & (T - 1)) || skip > file.size()) return 2;
  if (!strcmp(argv[1], "run") && argc == 8) {
    uint8_t* b = exact_copy(file, file.size());
    const Result r = tiled(b, file.size(), skip, n_ref, T, atoi(argv[6]) != 0);
    naive_check(b, file.size(), skip, r, "run");
    report(r);
    FILE* o = fopen(argv[7], "wb");
    if (!o) return 2;
    if (!r.starts.empty()) fwrite(r.starts.data(), 4, r.starts.size(), o);
    fclose(o);
    free(b);
  } else if (!strcmp(argv[1], "trunc")) {
    unsigned long long runs = 0;
    for (size_t n = skip; n <= file.size(); ++n) {
      uint8_t* b = exact_copy(file, n);
      for (int ng = 0; ng < 2; ++ng) {
        const Result r = tiled(b, n, skip, n_ref, T, ng != 0);
        naive_check(b, n, skip, r, "trunc");
        ++runs;
      }
      free(b);
    }
    printf("trunc ok %llu\n", runs);
  } else if (!strcmp(argv[1], "flips") && argc == 8) {
    uint32_t x = (uint32_t)atoi(argv[6]);
    const int count = atoi(argv[7]);
    unsigned long long refused = 0;
    for (int i = 0; i < count; ++i) {
      uint8_t* b = exact_copy(file, file.size());
      x = x * 1664525u + 1013904223u;
      const size_t at = skip + (x >> 4) % (file.size() - skip);
      x = x * 1664525u + 1013904223u;
      b[at] ^= (uint8_t)(1u + (x >> 8) % 255u);
      for (int ng = 0; ng < 2; ++ng) {
        const Result r = tiled(b, file.size(), skip, n_ref, T, ng != 0);
        naive_check(b, file.size(), skip, r, "flips");
        if (ng == 0 && r.status) ++refused;
      }
      free(b);
    }
    printf("flips ok %d refused %llu\n", count, refused);
  } else {
    return 2;
  }
  printf("refusals %llu %llu %llu %llu %llu\n", g_stats.refusals[1], g_stats.refusals[2], g_stats.refusals[3], g_stats.refusals[4],
         g_stats.refusals[5]);
  printf("wrong_guess %llu\n", g_stats.wrong_guess);
  return 0;
}
