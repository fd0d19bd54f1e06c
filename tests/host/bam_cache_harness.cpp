// Host harness over rufus_amd/csrc/host/rfx_bam_cache.hpp for tests/test_bam_cache_host.py, built with
// -fsanitize=address,undefined.  Nothing here touches a device.
//
//   read FILE ...      read_cache, a line per file: "ok chunks C records R blocks T names N ..." or "refused" (exit 0 either way)
//   copy IN OUT        read_cache(IN), then every part of it through Writer into OUT ("refused": exit 0, no OUT)
//   sam FILE           rfxcache::read_chunks (the SAM-kind reader) on FILE: "ok" or "refused"
//   plan FILE CAP      FILE: text -- n_blocks, then "csize isize" per block; n_sel, then "stream_off bytes" per record.
//                      plan_fetch: "error <text>" or, per batch, "batch <inflated> <first> <n>", "blocks <index> ...",
//                      "at <arena offset> ..."
#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include "../../rufus_amd/csrc/host/rfx_bam_cache.hpp"
#include "../../rufus_amd/csrc/host/rfx_packed_cache.hpp"

namespace {

// the file's bytes in memory aligned to 8 (as a mapping is), exactly `size` of them: the sanitizer sees a read behind them
struct Blob {
  uint64_t* mem = nullptr;
  size_t size = 0;
  const char* data() const { return (const char*)mem; }
  ~Blob() { delete[] mem; }
};
bool slurp(const char* path, Blob& b) {
  std::ifstream f(path, std::ios::binary);
  if (!f) return false;
  std::string s((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
  b.size = s.size();
  // (a size that is no multiple of 8 is refused before anything is read: the last word may be partly outside `size`)
  b.mem = new uint64_t[(s.size() + 7) / 8];
  memcpy(b.mem, s.data(), s.size());
  return true;
}

int cmd_read(const char* path) {
  Blob b;
  if (!slurp(path, b)) return 2;
  rfxbamcache::Cache c;
  if (!rfxbamcache::read_cache(b.data(), b.size, c)) {
    puts("refused");
    return 0;
  }
  // touch everything a reader indexes with
  uint64_t sum = 0, words = 0;
  for (const auto& ch : c.chunks) {
    for (uint32_t i = 0; i < ch.n; ++i) sum += ch.hash[i] + ch.start[i] + ch.rbytes[i] + ch.len[i] + ch.word_off[i + 1];
    for (uint32_t w = 0; w < ch.n_words; ++w) sum += ch.codes[w] + ch.good[w];
    for (uint32_t r = 0; r < 2 * ch.n_runs; ++r) sum += ch.runs[r];
    words += ch.n_words;
  }
  for (uint64_t i = 0; i < c.h.n_blocks; ++i) sum += c.index[i].file_off + c.index[i].csize;
  printf("ok chunks %zu records %llu blocks %llu names %zu words %llu min_q %d exclude %u bam %llu stream %llu sum %llu\n", c.chunks.size(),
         (unsigned long long)c.h.n_records, (unsigned long long)c.h.n_blocks, c.names.size(), (unsigned long long)words, c.h.min_q,
         c.h.exclude_flags, (unsigned long long)c.h.bam_bytes, (unsigned long long)c.h.stream_bytes, (unsigned long long)sum);
  return 0;
}

int cmd_copy(const char* in, const char* out_path) {
  Blob b;
  if (!slurp(in, b)) return 2;
  rfxbamcache::Cache c;
  if (!rfxbamcache::read_cache(b.data(), b.size, c)) {
    puts("refused");
    return 0;
  }
  const int fd = ::open(out_path, O_WRONLY | O_CREAT | O_TRUNC, 0644);
  if (fd < 0) return 2;
  std::string names;
  for (const auto& n : c.names) names.append(n).push_back('\0');
  rfxbamcache::Writer w;
  bool ok = w.open(fd, c.h.min_q, c.h.exclude_flags, c.h.n_ref, names.data(), names.size());
  for (const auto& ch : c.chunks) ok = ok && w.add_chunk(ch);
  for (uint64_t i = 0; i < c.h.n_blocks; ++i) w.add_block(c.index[i].csize, c.index[i].isize);
  ok = ok && w.finish();
  ok = (::close(fd) == 0) && ok;
  puts(ok ? "ok" : "write error");
  return ok ? 0 : 3;
}

int cmd_sam(const char* path) {
  Blob b;
  if (!slurp(path, b)) return 2;
  int min_q = 0;
  std::vector<rfxcache::ChunkView> chunks;
  // (the stream length a SAM-kind header would have to carry: whatever stands where that reader looks for it)
  uint64_t stream_bytes = 0;
  if (b.size >= sizeof(rfxcache::FileHeader)) memcpy(&stream_bytes, b.data() + offsetof(rfxcache::FileHeader, stream_bytes), 8);
  puts(rfxcache::read_chunks(b.data(), b.size, stream_bytes, min_q, chunks) ? "ok" : "refused");
  return 0;
}

int cmd_plan(const char* path, const char* cap) {
  std::ifstream f(path);
  if (!f) return 2;
  uint64_t n_blocks = 0, n_sel = 0;
  f >> n_blocks;
  std::vector<rfxbamcache::IndexEntry> index(n_blocks);
  uint64_t fo = 0, so = 0;
  for (auto& e : index) {
    f >> e.csize >> e.isize;
    e.file_off = fo, e.inflated_off = so;
    fo += e.csize, so += e.isize;
  }
  f >> n_sel;
  std::vector<rfxbamcache::Selected> sel(n_sel);
  for (auto& s : sel) f >> s.stream_off >> s.bytes;
  if (!f) return 2;
  std::vector<rfxbamcache::Batch> batches;
  std::string err;
  if (!rfxbamcache::plan_fetch(index.data(), n_blocks, so, sel, strtoull(cap, nullptr, 10), batches, &err)) {
    printf("error %s\n", err.c_str());
    return 0;
  }
  for (const auto& b : batches) {
    printf("batch %llu %zu %zu\nblocks", (unsigned long long)b.inflated, b.first, b.n);
    for (const uint64_t k : b.block) printf(" %llu", (unsigned long long)k);
    printf("\nat");
    for (const uint32_t a : b.arena_off) printf(" %u", a);
    printf("\n");
  }
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  const std::string cmd = argc > 1 ? argv[1] : "";
  if (cmd == "read" && argc >= 3) {
    for (int i = 2; i < argc; ++i)
      if (const int rc = cmd_read(argv[i])) return rc;
    return 0;
  }
  if (cmd == "copy" && argc == 4) return cmd_copy(argv[2], argv[3]);
  if (cmd == "sam" && argc == 3) return cmd_sam(argv[2]);
  if (cmd == "plan" && argc == 4) return cmd_plan(argv[2], argv[3]);
  fprintf(stderr, "usage: bam_cache_harness read FILE ... | copy IN OUT | sam FILE | plan FILE CAP\n");
  return 2;
}
