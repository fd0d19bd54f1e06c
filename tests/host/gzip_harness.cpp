// Stand-alone host harness of the plain-gzip route of `jellyfish count` (rufus_amd/csrc/rfx_gzip_core.h: the statements the
// kernels of rfx_gzip.hip run, and the chain rule gz_append the library runs on the host; rufus_amd/csrc/host/
// rfx_ingest.hpp, class GzipIngest), built plain and with -fsanitize=address,undefined by tests/test_gzip_host.py.  TEST
// INFRASTRUCTURE: nothing here is built into the product, whose jellyfish has no CPU path.
//
// The backend below does serially what the kernels do: the finder (gz_prefilter at every bit offset behind a nominal
// boundary, gz_probe on the survivors), the walk (gz_run with nothing stored), the marker inflate (gz_run with the 16-bit
// policy), the windows (each chunk's last 32 KiB in order), the resolve (every value through its chunk's window) and the
// CRC (lane slices of 64 KiB segments, shifted to the chunk's end and XORed).  The input is a heap copy of exactly the
// presented bytes (a read past it is AddressSanitizer's); every buffer that is written -- arena, 16-bit side buffer, the
// two window buffers -- has 64 guard bytes on both sides, checked after every call.
//
//   gzip_harness core CHUNK_BYTES PIECE_BYTES ARENA_BYTES FILE...
// presents each FILE to rfx_text_append_gzip (the stand-in: gz_append over the backend) in pieces of PIECE_BYTES, from
// `consumed` on; a piece that holds no whole chunk doubles; a full arena is emptied into the output.  Prints per file
//   file NAME / format <text>  or  crc <hex> bytes <n> / stats <8 numbers> / prefilter <passed> probes <passed> / starts <bits...>
//   / guards ok
//
//   gzip_harness ingest ARENA_BYTES PIECE_BYTES CHUNK_BYTES FILE...
// runs GzipIngest as the executable uses it over stand-ins for the arenas (byte vectors; settle and parse as
// tests/host/fasta_harness.cpp's FASTQ mode).  Prints `A <bytes> <crc>` per arena sunk, `ok <the route's counts>` per file
// and `text crc <hex> bytes <n> records <r>` at the end.  What the driver refuses ends the process with its message and
// exit 1.  Build with
//   g++ -O1 -g -std=c++17 -pthread gzip_harness.cpp ../../rufus_amd/csrc/rfx_host.cpp
#include <cstdlib>
#include <fstream>
#include <vector>

#include "../../rufus_amd/csrc/host/rfx_ingest.hpp"
#include "../../rufus_amd/csrc/rfx_gzip_core.h"

static std::string g_error = "host stand-in";
static uint32_t g_chunk = 1u << 16;
static uint64_t g_prefilter = 0, g_probe = 0;
static bool g_guards = true;

struct Guarded {
  std::vector<uint8_t> raw;
  size_t n = 0;
  void init(size_t bytes, uint8_t fill) {
    n = bytes;
    raw.assign(bytes + 128, 0xA5);
    std::fill(raw.begin() + 64, raw.begin() + 64 + (long)bytes, fill);
  }
  uint8_t* p() { return raw.data() + 64; }
  const uint8_t* p() const { return raw.data() + 64; }
  void check() const {
    for (size_t i = 0; i < 64; ++i)
      if (raw[i] != 0xA5 || raw[64 + n + i] != 0xA5) g_guards = false;
  }
};

struct rfx_ctx { int device; };
struct rfx_reads { std::vector<uint8_t> text; uint32_t n = 0; };
struct rfx_text {
  Guarded arena;
  uint64_t cap = 0, used = 0;
  long tickets = 0;
};
struct rfx_gzip {
  gz_stream S;
  Guarded win[2];
  int cur = 0;
};

struct host_backend {
  rfx_gzip* g;
  rfx_text* t;
  std::vector<uint8_t> in;  // exactly the presented bytes
  uint64_t n;
  bgzf_tables tables;

  uint64_t room() const { return t->cap - t->used; }
  uint64_t cap() const { return t->cap; }

  int find(uint64_t first_boundary, uint32_t chunk_bytes, std::vector<uint64_t>& out) {
    const uint8_t* p = in.data();
    for (uint64_t b = first_boundary; b < n; b += chunk_bytes) {
      const uint64_t lo_bit = b * 8u, hi_bit = std::min(lo_bit + (uint64_t)chunk_bytes * 8u, n * 8u);
      for (uint64_t bit = lo_bit; bit < hi_bit; ++bit) {
        uint64_t lo, hi;
        gz_bits128(p, p + n, bit, &lo, &hi);
        if (!gz_prefilter(lo, hi)) continue;
        ++g_prefilter;
        if (gz_probe(p, p + n, bit, tables)) {
          ++g_probe;
          out.push_back(bit);
          break;
        }
      }
    }
    return 0;
  }

  int walk(std::vector<gz_chunk>& list, const std::vector<uint32_t>& which) {
    const uint8_t* p = in.data();
    for (uint32_t i : which) {
      gz_null_out no;
      gz_run(p, p + n, list[i].start, list[i].stop, list[i].first != 0u, ~0ull, tables, no, list[i].res);
    }
    return 0;
  }

  int inflate(const gz_chunk* k, size_t nk, uint64_t total, uint32_t* crc_reg) {
    if (total > room()) return RFX_E_RANGE;
    if (total == 0) return 0;
    const uint8_t* p = in.data();
    Guarded side;
    side.init((size_t)total * 2, 0xEE);
    uint16_t* s16 = (uint16_t*)side.p();
    std::vector<uint64_t> off(nk + 1, 0);
    for (size_t i = 0; i < nk; ++i) off[i + 1] = off[i] + k[i].res.out_bytes;
    for (size_t i = 0; i < nk; ++i) {  // k_gz_inflate
      gz_serial16 so{s16 + off[i]};
      gz_result r;
      gz_run(p, p + n, k[i].start, k[i].stop, k[i].first != 0u, k[i].res.out_bytes, tables, so, r);
      if (r.status != BGZF_OK || r.out_bytes != k[i].res.out_bytes || r.end_bit != k[i].res.end_bit) {
        g_error = "rfx_text_append_gzip: the inflate of a chunk does not repeat its walk";
        return RFX_E_HIP;
      }
    }
    uint8_t* out = t->arena.p() + t->used;
    const uint8_t* win = g->win[g->cur].p();
    uint8_t* win_next = g->win[g->cur ^ 1].p();
    for (size_t i = 0; i < nk; ++i) {  // k_gz_windows
      const uint64_t nb = k[i].res.out_bytes;
      for (uint64_t q = nb > GZ_WINDOW ? nb - GZ_WINDOW : 0; q < nb; ++q) out[off[i] + q] = gz_resolve16(s16[off[i] + q], out, win, off[i]);
    }
    for (uint32_t q = 0; q < GZ_WINDOW; ++q) {
      const uint64_t idx = total + q;
      win_next[q] = idx < GZ_WINDOW ? win[idx] : out[idx - GZ_WINDOW];
    }
    for (size_t i = nk; i-- > 0;)  // k_gz_resolve (in no particular order: here from the back)
      for (uint64_t q = 0; q < k[i].res.out_bytes; ++q) out[off[i] + q] = gz_resolve16(s16[off[i] + q], out, win, off[i]);
    for (size_t i = 0; i < nk; ++i) {  // k_gz_crc
      const uint64_t nb = k[i].res.out_bytes;
      uint32_t x = 0;
      for (uint64_t seg_lo = 0; seg_lo < nb; seg_lo += 65536) {
        const uint32_t len = (uint32_t)std::min<uint64_t>(65536, nb - seg_lo), slice = (len + 63u) / 64u;
        for (uint32_t lane = 0; lane < 64u; ++lane) {
          const uint32_t lo = lane * slice < len ? lane * slice : len, hi = lo + slice < len ? lo + slice : len;
          const uint32_t reg = bgzf_crc_update(0u, out + off[i] + seg_lo + lo, hi - lo);
          x ^= bgzf_crc_shift(reg, (uint32_t)(nb - seg_lo - hi));
        }
      }
      crc_reg[i] = x;
    }
    side.check();
    g->cur ^= 1;
    t->used += total;
    return 0;
  }
};

extern "C" {

const char* rfx_last_error(void) { return g_error.c_str(); }
void rfx_reads_free(rfx_reads* r) { delete r; }
uint32_t rfx_reads_count(const rfx_reads* r) { return r ? r->n : 0; }

rfx_text* rfx_text_open(rfx_ctx*, uint64_t cap_bytes) {
  rfx_text* t = new rfx_text;
  t->cap = cap_bytes;
  t->arena.init((size_t)cap_bytes, 0);
  return t;
}
void rfx_text_close(rfx_text* t) {
  t->arena.check();
  delete t;
}
uint64_t rfx_text_room(const rfx_text* t) { return t->cap - t->used; }
uint64_t rfx_text_bytes(const rfx_text* t) { return t->used; }
long rfx_text_append(rfx_text* t, const void* host, uint64_t n) {
  if (n > rfx_text_room(t)) return RFX_E_RANGE;
  memcpy(t->arena.p() + t->used, host, n);
  t->used += n;
  return t->tickets++;
}
int rfx_text_wait(rfx_text* t, long ticket) { return ticket >= 0 && ticket < t->tickets ? RFX_OK : RFX_E_INVAL; }
void rfx_text_reset(rfx_text* t) {
  t->arena.check();
  t->used = 0;
  t->tickets = 0;
}
int rfx_text_settle(rfx_text* t, rfx_text* next, uint64_t* carried) {
  *carried = 0;
  if (next == t || (next && next->used)) return RFX_E_INVAL;
  uint64_t lines = 0, cut = 0;
  for (uint64_t i = 0; i < t->used; ++i)
    if (t->arena.p()[i] == '\n' && (++lines & 3u) == 0) cut = i + 1;
  const uint64_t tail = t->used - cut;
  if (tail) {
    if (!next) return RFX_E_FORMAT;
    if (tail > next->cap) return RFX_E_RANGE;
    memcpy(next->arena.p(), t->arena.p() + cut, tail);
    next->used = tail;
  }
  t->used = cut;
  *carried = tail;
  return RFX_OK;
}
rfx_reads* rfx_text_parse(rfx_text* t, int flags, int, int* strict) {
  *strict = 1;
  if (flags != RFX_PACK_COUNT) return nullptr;
  const uint8_t* x = t->arena.p();
  const uint64_t n = t->used;
  std::vector<uint64_t> ls{0};
  for (uint64_t i = 0; i < n; ++i)
    if (x[i] == '\n') ls.push_back(i + 1);
  const uint64_t lines = ls.size() - 1;
  *strict = 0;
  if (n == 0 || x[n - 1] != '\n' || lines == 0 || (lines & 3)) return nullptr;
  for (uint64_t r = 0; r < lines / 4; ++r) {
    const uint64_t l0 = ls[4 * r], l1 = ls[4 * r + 1], l2 = ls[4 * r + 2], l3 = ls[4 * r + 3], l4 = ls[4 * r + 4];
    if (!(l1 - l0 >= 2 && x[l0] == '@' && l3 - l2 >= 2 && x[l2] == '+' && l2 - 1 - l1 == l4 - 1 - l3)) return nullptr;
  }
  *strict = 1;
  rfx_reads* rd = new rfx_reads;
  rd->text.assign(x, x + n);
  rd->n = (uint32_t)(lines / 4);
  return rd;
}

rfx_gzip* rfx_gzip_open(rfx_ctx*) {
  rfx_gzip* g = new rfx_gzip;
  g->S.e_format = RFX_E_FORMAT;
  g->S.chunk_bytes = g_chunk;
  for (Guarded& w : g->win) w.init(GZ_WINDOW, 0);
  return g;
}
void rfx_gzip_close(rfx_gzip* g) {
  for (const Guarded& w : g->win) w.check();
  delete g;
}
long rfx_text_append_gzip(rfx_text* t, rfx_gzip* g, const void* host, uint64_t n, int eof, uint64_t* consumed) {
  std::unique_ptr<host_backend> B(new host_backend{g, t, std::vector<uint8_t>((const uint8_t*)host, (const uint8_t*)host + n), n, {}});
  const long rc = gz_append(g->S, *B, B->in.data(), n, eof != 0, consumed);
  if (rc == RFX_E_FORMAT && !g->S.msg.empty()) g_error = g->S.msg;
  t->arena.check();
  for (const Guarded& w : g->win) w.check();
  return rc;
}
int rfx_gzip_stats(const rfx_gzip* g, uint64_t out[8]) {
  for (int i = 0; i < 8; ++i) out[i] = g->S.stats[i];
  return RFX_OK;
}
uint64_t rfx_gzip_need(const rfx_gzip* g) { return g->S.need; }

}  // extern "C"

static std::vector<uint8_t> read_file(const char* path) {
  std::ifstream f(path, std::ios::binary);
  if (!f) rfxcli::die(std::string("cannot open ") + path);
  return std::vector<uint8_t>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}

int main(int argc, char** argv) {
  if (argc >= 6 && !strcmp(argv[1], "core")) {
    g_chunk = (uint32_t)atoll(argv[2]);
    const size_t piece0 = (size_t)atoll(argv[3]), arena = (size_t)atoll(argv[4]);
    rfx_ctx ctx{0};
    for (int a = 5; a < argc; ++a) {
      const std::vector<uint8_t> file = read_file(argv[a]);
      printf("file %s\n", argv[a]);
      g_prefilter = g_probe = 0;
      g_guards = true;
      rfx_text* t = rfx_text_open(&ctx, arena);
      rfx_gzip* g = rfx_gzip_open(&ctx);
      uint32_t reg = 0xFFFFFFFFu;
      uint64_t bytes = 0;
      auto empty = [&] {
        reg = bgzf_crc_update(reg, t->arena.p(), (uint32_t)t->used);
        bytes += t->used;
        rfx_text_reset(t);
      };
      size_t at = 0, piece = piece0;
      bool bad = false;
      while (at < file.size() || file.empty()) {
        const size_t n = std::min(piece, file.size() - at);
        uint64_t used = 0;
        const long got = rfx_text_append_gzip(t, g, file.data() + at, n, at + n == file.size(), &used);
        if (got < 0) {
          printf("format %ld %s\n", got, rfx_last_error());
          bad = true;
          break;
        }
        at += (size_t)used;
        if (file.empty()) break;
        if (got || used) continue;
        if (rfx_gzip_need(g)) empty();
        else if (n == file.size() - at) { printf("format 0 no progress at the end of the file\n"); bad = true; break; }
        else piece *= 2;
      }
      if (!bad) {
        empty();
        printf("crc %08x bytes %llu\n", ~reg, (unsigned long long)bytes);
      }
      printf("stats");
      for (int i = 0; i < 8; ++i) printf(" %llu", (unsigned long long)g->S.stats[i]);
      printf("\nprefilter %llu probes %llu\nstarts", (unsigned long long)g_prefilter, (unsigned long long)g_probe);
      for (uint64_t s : g->S.starts) printf(" %llu", (unsigned long long)s);
      printf("\n");
      rfx_gzip_close(g);
      rfx_text_close(t);
      printf("guards %s\n", g_guards ? "ok" : "BAD");
    }
    return 0;
  }
  if (argc >= 6 && !strcmp(argv[1], "ingest")) {
    const size_t arena = (size_t)atoll(argv[2]), piece = (size_t)atoll(argv[3]);
    g_chunk = (uint32_t)atoll(argv[4]);
    rfx_ctx ctx{0};
    uint32_t reg = 0xFFFFFFFFu;
    uint64_t bytes = 0, records = 0;
    {
      rfxcli::GzipIngest route(&ctx, [&](rfx_reads* r) {
        printf("A %zu %08x\n", r->text.size(), ~bgzf_crc_update(0xFFFFFFFFu, r->text.data(), (uint32_t)r->text.size()));
        reg = bgzf_crc_update(reg, r->text.data(), (uint32_t)r->text.size());
        bytes += r->text.size();
        records += r->n;
        rfx_reads_free(r);
      }, arena, piece);
      for (int a = 5; a < argc; ++a) {
        const std::vector<uint8_t> gz = read_file(argv[a]);
        route.feed_mapped((const char*)gz.data(), gz.size());
        printf("ok %s\n", route.counts().c_str());
      }
    }
    printf("text crc %08x bytes %llu records %llu\nguards %s\n", ~reg, (unsigned long long)bytes, (unsigned long long)records,
           g_guards ? "ok" : "BAD");
    return 0;
  }
  fprintf(stderr, "usage: gzip_harness core CHUNK PIECE ARENA FILE... | gzip_harness ingest ARENA PIECE CHUNK FILE...\n");
  return 2;
}
