// Host-only harness for `RUFUS.Filter.single --sam` and for the host tail of `RUFUS.Filter.single --bam`
// (rufus_amd/csrc/host/rufus_filter_main.cpp with -DRFX_SINGLE_END, rufus_amd/csrc/host/rfx_bam_single.hpp), a stand-alone
// program for the sanitizers:
//   filter_single_harness --sam CHRFILE HashList SAM|stdin STUB K MinQ Threshold Threads
//       the tool's own main() with the DEVICE entry points of the C-ABI replaced by host stand-ins, so that the reader, the
//       helper threads, the pieces handed over and recycled and the ordered `:MH` output run in the CPU suite
//   filter_single_harness --tail RECORDS HITS OUT
//       RECORDS: gathered BAM records one behind the other, as rfx_bam_gather_hits leaves them; HITS: a little-endian
//       uint32 per record.  Both are read into heap blocks of exactly their size, so that a read past a cut record is a
//       heap overflow the sanitizer sees.  OUT = BamSingleTail::add's text; a refusal: "rfx_bam_single: <why>" on stderr,
//       exit status 3, OUT holds the records in front of the bad one.
// TEST INFRASTRUCTURE: the stand-in for rfx_filter is a plain loop over the packed block (src/RUFUS.Filter.ss.cpp:176-193
// on the arrays rfx_pack_spans made); nothing here is built into the product, whose tools have no CPU path.  The host half
// of the library (rfx_hashlist_keys, rfx_pack_spans, rfx_host_cpus) is the real one: build with
//   g++ -std=c++17 -pthread -DRFX_SINGLE_END -fsanitize=... filter_single_harness.cpp ../../rufus_amd/csrc/rfx_host.cpp
#include <cstdlib>
#include <unordered_set>
#include <vector>

#ifndef RFX_SINGLE_END
#error "build with -DRFX_SINGLE_END: this is the single-end tool's harness"
#endif
#define main rfx_tool_main
#include "../../rufus_amd/csrc/host/rufus_filter_main.cpp"
#undef main

struct rfx_ctx { int device; };
struct rfx_set {
  std::unordered_set<uint64_t> keys;
  int k;
};
struct rfx_reads {
  std::vector<uint64_t> codes;
  std::vector<uint32_t> good, woff, len;
};

extern "C" {

const char* rfx_last_error(void) { return "host stand-in"; }
rfx_ctx* rfx_open(int device, size_t) { return new rfx_ctx{device}; }
void rfx_close(rfx_ctx* c) { delete c; }
int rfx_ctx_allow_peers(rfx_ctx*, const int*, int) { return RFX_OK; }
void* rfx_host_alloc(size_t bytes) { return malloc(bytes); }
void* rfx_host_alloc_lazy(size_t bytes) { return malloc(bytes); }
int rfx_host_pin(void*) { return RFX_OK; }
void rfx_host_free(void* p) { free(p); }

rfx_set* rfx_set_build(rfx_ctx*, const uint64_t* fwd_keys, uint64_t n, int k) {
  rfx_set* s = new rfx_set;
  s->k = k;
  s->keys.insert(fwd_keys, fwd_keys + n);
  return s;
}
void rfx_set_free(rfx_set* s) { delete s; }

rfx_reads* rfx_reads_upload(rfx_ctx*, const uint64_t* codes, const uint32_t*, const uint32_t* good, const uint32_t* word_off,
                            const uint32_t* len, uint32_t n_reads) {
  rfx_reads* r = new rfx_reads;
  const uint32_t words = word_off[n_reads];
  r->codes.assign(codes, codes + words);
  r->good.assign(good, good + words);
  r->woff.assign(word_off, word_off + n_reads + 1);
  r->len.assign(len, len + n_reads);
  return r;
}
void rfx_reads_free(rfx_reads* r) { delete r; }

// hits of a read = positions i < L - last_base_skipped that end a streak of >= k good bases and whose window (first
// base most significant, 2 bits per base) is in the set
int rfx_filter(rfx_set* s, const rfx_reads* r, int thresh, int last_base_skipped, uint32_t* hits_out, uint64_t* hitmask_out,
               uint64_t* n_hit_reads) {
  const int k = s->k;
  const uint64_t kmask = k >= 32 ? ~0ull : (1ull << (2 * k)) - 1;
  const size_t n = r->len.size();
  uint64_t over = 0;
  if (hitmask_out)
    for (size_t w = 0; w < (n + 63) / 64; ++w) hitmask_out[w] = 0;
  for (size_t x = 0; x < n; ++x) {
    const uint32_t L = r->len[x], w0 = r->woff[x];
    const uint32_t stop = last_base_skipped ? (L ? L - 1 : 0) : L;
    uint64_t key = 0;
    int streak = 0;
    uint32_t found = 0;
    for (uint32_t i = 0; i < stop; ++i) {
      const uint64_t code = (r->codes[w0 + i / 32] >> (2 * (i % 32))) & 3u;
      const bool good = (r->good[w0 + i / 32] >> (i % 32)) & 1u;
      key = ((key << 2) | code) & kmask;
      streak = good ? streak + 1 : 0;
      if (streak >= k && s->keys.count(key)) ++found;
    }
    if (hits_out) hits_out[x] = found;
    if ((int)found >= thresh) {
      ++over;
      if (hitmask_out) hitmask_out[x >> 6] |= 1ull << (x & 63);
    }
  }
  if (n_hit_reads) *n_hit_reads = over;
  return RFX_OK;
}

}  // extern "C"

// a file's bytes in a heap block of exactly its size (nullptr for an empty file)
static uint8_t* exact_copy(const char* path, size_t* n) {
  FILE* f = fopen(path, "rb");
  if (!f) {
    fprintf(stderr, "filter_single_harness: cannot open %s\n", path);
    exit(2);
  }
  fseek(f, 0, SEEK_END);
  *n = (size_t)ftell(f);
  fseek(f, 0, SEEK_SET);
  uint8_t* p = *n ? (uint8_t*)malloc(*n) : nullptr;
  if (*n && fread(p, 1, *n, f) != *n) exit(2);
  fclose(f);
  return p;
}

static int run_tail(const char* records, const char* hits, const char* out_path) {
  size_t nb = 0, nh = 0;
  uint8_t* b = exact_copy(records, &nb);
  uint8_t* h = exact_copy(hits, &nh);
  rfxsam::BamSingleTail tail;
  std::string why;
  const bool ok = tail.add(b, nb, (const uint32_t*)h, nh / 4, &why);
  FILE* o = fopen(out_path, "wb");
  if (!o) exit(2);
  fwrite(tail.out.data(), 1, tail.out.size(), o);
  fclose(o);
  free(b);
  free(h);
  if (!ok) {
    fprintf(stderr, "rfx_bam_single: %s\n", why.c_str());
    return 3;
  }
  printf("records %llu windows %llu\n", (unsigned long long)tail.records, (unsigned long long)tail.windows);
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 5 && strcmp(argv[1], "--tail") == 0) return run_tail(argv[2], argv[3], argv[4]);
  return rfx_tool_main(argc, argv);
}
