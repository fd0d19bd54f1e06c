// Stand-alone host harness of the bgzip'd-FASTA route of `jellyfish count` (rufus_amd/csrc/rfx_fasta_core.h, the rule the
// kernels of rfx_fasta.hip run; rufus_amd/csrc/host/rfx_ingest.hpp, class BgzfIngest in its FASTA mode), built plain and
// with -fsanitize=address,undefined by tests/test_fasta_host.py.  TEST INFRASTRUCTURE: nothing here is built into the
// product, whose jellyfish has no CPU path.
//
//   fasta_harness core [--trunc] FILE...
// runs the host side of the core over each FILE's bytes (--trunc: over every prefix of them) the way the kernels do --
// line starts, fa_line_key per line, the two scans, the compacted list of non-empty sequence lines, fa_pack_word per
// output code word -- on heap copies of exactly the text's size, and prints per text
//   T <bytes> <1: FASTA, 0: does not begin with '>'> n <reads> max <longest> len <..> off <..> codes <hex..> mask <hex..>
//
//   fasta_harness ingest ARENA_BYTES PIECE_BYTES FILE.gz...
// runs the ingest class as the executable uses it -- every file sniffed by bgzf_first_byte, '>' to the FASTA mode,
// anything else to the FASTQ mode -- over HOST stand-ins for the device entry points: arenas are byte vectors,
// rfx_text_append_bgzf is the host side of rfx_bgzf_core.h, rfx_text_settle_fasta / rfx_text_parse_fasta are the core as
// above.  Prints `settle <bytes before> <carried>` for every FASTA settle, `R <len> <crc32 of the read's code words then
// mask words>` for every read sunk, and `ok <the route's counts>` per file.  What the driver refuses ends the process with
// its message and exit 1 (die()).  The host half of the library is the real one (rfx_bgzf_scan, rfx_pack_spans): build with
//   g++ -O1 -g -std=c++17 -pthread fasta_harness.cpp ../../rufus_amd/csrc/rfx_host.cpp
#include <fcntl.h>

#include <cstdlib>
#include <fstream>
#include <vector>

#include "../../rufus_amd/csrc/host/rfx_ingest.hpp"
#include "../../rufus_amd/csrc/rfx_bgzf_core.h"
#include "../../rufus_amd/csrc/rfx_fasta_core.h"

struct rfx_ctx { int device; };
struct rfx_reads {
  std::vector<uint64_t> codes;
  std::vector<uint32_t> acgt, woff, len;
  uint32_t max_len = 0;
};
struct rfx_text {
  std::vector<uint8_t> text;
  uint64_t cap = 0;
  uint32_t n_blocks = 0;
  bool failed = false;
  long tickets = 0;
};

static std::string g_error = "host stand-in";

// ---- the core, driven serially the way rfx_fasta.hip drives it ----------------------------------------------------------
// false: the text is empty or does not begin with '>'
static bool pack_text(const uint8_t* src, uint64_t n, rfx_reads& out) {
  std::vector<uint8_t> copy(src, src + n);  // (a heap block of exactly the text's size: a read past it is ASan's)
  const uint8_t* t = copy.data();
  if (n == 0 || t[0] != '>') return false;
  std::vector<uint32_t> ls{0};  // k_txt_lines: the byte behind every newline
  for (uint64_t i = 0; i < n; ++i)
    if (t[i] == '\n') ls.push_back((uint32_t)(i + 1));
  const uint64_t n_nl = ls.size() - 1, n_lines = n_nl + (t[n - 1] != '\n' ? 1 : 0);
  std::vector<uint64_t> key(n_lines + 1), ne(n_lines + 1);
  for (uint64_t i = 0; i < n_lines; ++i) {  // k_fa_lines
    const uint64_t b = ls[i], e = i < n_nl ? (uint64_t)ls[i + 1] - 1u : n;
    key[i] = fa_line_key(t, n, b, e);
    ne[i] = fa_key_bases(key[i]) ? 1u : 0u;
  }
  auto scan = [](std::vector<uint64_t>& v, uint64_t m) {  // exclusive, v[m] = total
    uint64_t run = 0;
    for (uint64_t i = 0; i < m; ++i) {
      const uint64_t x = v[i];
      v[i] = run;
      run += x;
    }
    v[m] = run;
  };
  scan(key, n_lines);
  scan(ne, n_lines);
  const uint32_t n_rec = fa_key_headers(key[n_lines]), n_ne = (uint32_t)ne[n_lines];
  std::vector<uint32_t> rec_base(n_rec + 1), ne_base(n_ne + 1), ne_src(n_ne + 1);
  rec_base[n_rec] = ne_base[n_ne] = fa_key_bases(key[n_lines]);
  for (uint64_t i = 0; i < n_lines; ++i) {  // k_fa_scatter
    const uint64_t at = key[i], mine = key[i + 1] - at;
    if (fa_key_headers(mine)) rec_base.at(fa_key_headers(at)) = fa_key_bases(at);
    else if (fa_key_bases(mine)) {
      ne_base.at(ne[i]) = fa_key_bases(at);
      ne_src.at(ne[i]) = ls[i];
    }
  }
  std::vector<uint64_t> words(n_rec + 1);
  out.len.assign(n_rec, 0);
  out.max_len = 0;
  for (uint32_t r = 0; r < n_rec; ++r) {  // k_fa_reads
    out.len[r] = rec_base[r + 1] - rec_base[r];
    words[r] = (out.len[r] + 31u) / 32u;
    out.max_len = std::max(out.max_len, out.len[r]);
  }
  scan(words, n_rec);
  const uint64_t n_words = words[n_rec];
  out.woff.assign(n_rec + 1, 0);
  out.codes.assign(n_words, 0);
  out.acgt.assign(n_words, 0);
  for (uint32_t r = 0; r <= n_rec; ++r) out.woff[r] = (uint32_t)words[r];
  for (uint64_t w = 0; w < n_words; ++w) {  // k_fa_pack
    const uint32_t r = fa_last_le_u64(words.data(), n_rec, w);
    const uint64_t j = w - words[r];
    const uint32_t first = rec_base[r], L = rec_base[r + 1] - first, done = (uint32_t)j * 32u;
    uint64_t c = 0;
    uint32_t m = 0;
    if (j * 32u < L) fa_pack_word(t, n, ne_base.data(), ne_src.data(), n_ne, first + done, std::min(32u, L - done), &c, &m);
    out.codes[w] = c;
    out.acgt[w] = m;
  }
  return true;
}

static void print_block(uint64_t n, bool fasta, const rfx_reads& b) {
  printf("T %llu %d", (unsigned long long)n, (int)fasta);
  if (fasta) {
    printf(" n %zu max %u len", b.len.size(), b.max_len);
    for (uint32_t l : b.len) printf(" %u", l);
    printf(" off");
    for (uint32_t o : b.woff) printf(" %u", o);
    printf(" codes");
    for (uint64_t c : b.codes) printf(" %llx", (unsigned long long)c);
    printf(" mask");
    for (uint32_t m : b.acgt) printf(" %x", m);
  }
  printf("\n");
}

static void print_reads(const rfx_reads& b) {
  for (size_t r = 0; r < b.len.size(); ++r) {
    const uint32_t w0 = b.woff[r], w1 = b.woff[r + 1];
    uint32_t reg = bgzf_crc_update(0xFFFFFFFFu, (const uint8_t*)(b.codes.data() + w0), (w1 - w0) * 8u);
    reg = bgzf_crc_update(reg, (const uint8_t*)(b.acgt.data() + w0), (w1 - w0) * 4u);
    printf("R %u %u\n", b.len[r], ~reg);
  }
}

struct SerialOut {
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

static uint32_t inflate_block(const uint8_t* b, uint32_t pay_off, uint32_t pay_len, uint32_t isize, uint32_t crc, std::vector<uint8_t>& out) {
  static bgzf_tables* tables = new bgzf_tables();
  std::vector<uint8_t> in(b + pay_off, b + pay_off + pay_len);
  out.assign(isize, 0);
  SerialOut so{out.data()};
  uint32_t st = bgzf_inflate(in.data(), in.data() + in.size(), isize, *tables, so);
  if (st == BGZF_OK && ~bgzf_crc_update(0xFFFFFFFFu, out.data(), isize) != crc) st = BGZF_E_CRC;
  return st;
}

static std::vector<uint64_t> line_starts(const uint8_t* t, uint64_t n) {
  std::vector<uint64_t> ls{0};
  for (uint64_t i = 0; i < n; ++i)
    if (t[i] == '\n') ls.push_back(i + 1);
  return ls;
}

static int cut_text(rfx_text* t, rfx_text* next, uint64_t cut, uint64_t* carried) {
  const uint64_t tail = t->text.size() - cut;
  if (tail) {
    if (!next) return RFX_E_FORMAT;
    if (tail > next->cap) return RFX_E_RANGE;
    next->text.assign(t->text.begin() + (long)cut, t->text.end());
  }
  t->text.resize(cut);
  t->text.shrink_to_fit();
  *carried = tail;
  return RFX_OK;
}

extern "C" {

const char* rfx_last_error(void) { return g_error.c_str(); }
void* rfx_host_alloc(size_t bytes) { return malloc(bytes); }
void rfx_host_free(void* p) { free(p); }
void rfx_reads_free(rfx_reads* r) { delete r; }
uint32_t rfx_reads_count(const rfx_reads* r) { return r ? (uint32_t)r->len.size() : 0; }

rfx_text* rfx_text_open(rfx_ctx*, uint64_t cap_bytes) {
  rfx_text* t = new rfx_text;
  t->cap = cap_bytes;
  return t;
}
void rfx_text_close(rfx_text* t) { delete t; }
uint64_t rfx_text_room(const rfx_text* t) { return t->cap - t->text.size(); }
uint64_t rfx_text_bytes(const rfx_text* t) { return t->text.size(); }
long rfx_text_append(rfx_text* t, const void* host, uint64_t n) {
  if (n > rfx_text_room(t)) return RFX_E_RANGE;
  t->text.insert(t->text.end(), (const uint8_t*)host, (const uint8_t*)host + n);
  return t->tickets++;
}
int rfx_text_wait(rfx_text* t, long ticket) { return ticket >= 0 && ticket < t->tickets ? RFX_OK : RFX_E_INVAL; }
void rfx_text_reset(rfx_text* t) {
  t->text.clear();
  t->text.shrink_to_fit();
  t->n_blocks = 0;
  t->failed = false;
  t->tickets = 0;
}
long rfx_text_append_bgzf(rfx_text* t, const void* host, uint64_t n) {
  uint32_t nb = 0;
  uint64_t consumed = 0, inflated = 0;
  if (rfx_bgzf_scan(host, n, 0xFFFFFFFFu, &nb, &consumed, &inflated) != RFX_OK || consumed != n) return RFX_E_FORMAT;
  if (inflated > rfx_text_room(t)) return RFX_E_RANGE;
  std::vector<uint8_t> copy((const uint8_t*)host, (const uint8_t*)host + n), out;
  uint64_t at = 0;
  for (uint32_t i = 0; i < nb; ++i) {
    uint32_t bsize, pay_off, pay_len, isize, crc;
    (void)bgzf_block_header(copy.data() + at, n - at, &bsize, &pay_off, &pay_len, &isize, &crc);
    const uint32_t st = inflate_block(copy.data() + at, pay_off, pay_len, isize, crc, out);
    if (st != BGZF_OK && !t->failed) {
      t->failed = true;
      char msg[160];
      snprintf(msg, sizeof msg, "rfx_bgzf: block %u: %s", t->n_blocks + i, bgzf_status_text(st));
      g_error = msg;
    }
    t->text.insert(t->text.end(), out.begin(), out.end());
    at += bsize;
  }
  t->n_blocks += nb;
  return t->tickets++;
}

// the FASTQ mode's two (rfx_text.hip): the cut behind the last whole group of four lines; strict 4-line records
int rfx_text_settle(rfx_text* t, rfx_text* next, uint64_t* carried) {
  *carried = 0;
  if (next == t || (next && !next->text.empty())) return RFX_E_INVAL;
  if (t->failed) return RFX_E_FORMAT;
  const std::vector<uint64_t> ls = line_starts(t->text.data(), t->text.size());
  return cut_text(t, next, ls[(ls.size() - 1) / 4 * 4], carried);
}
rfx_reads* rfx_text_parse(rfx_text* t, int flags, int, int* strict) {
  *strict = 1;
  if (t->failed || flags != RFX_PACK_COUNT) return nullptr;
  const uint8_t* x = t->text.data();
  const uint64_t n = t->text.size();
  const std::vector<uint64_t> ls = line_starts(x, n);
  const uint64_t lines = ls.size() - 1;
  *strict = 0;
  if (n == 0 || x[n - 1] != '\n' || lines == 0 || (lines & 3)) return nullptr;
  const uint64_t nr = lines / 4;
  std::vector<uint64_t> so(nr);
  std::vector<uint32_t> sl(nr);
  uint64_t words = 0;
  for (uint64_t r = 0; r < nr; ++r) {
    const uint64_t l0 = ls[4 * r], l1 = ls[4 * r + 1], l2 = ls[4 * r + 2], l3 = ls[4 * r + 3], l4 = ls[4 * r + 4];
    const uint64_t L = l2 - 1 - l1, Q = l4 - 1 - l3;
    if (!(l1 - l0 >= 2 && x[l0] == '@' && l3 - l2 >= 2 && x[l2] == '+' && L == Q)) return nullptr;
    so[r] = l1;
    sl[r] = (uint32_t)L;
    words += (L + 31) / 32;
  }
  *strict = 1;
  rfx_reads* rd = new rfx_reads;
  rd->codes.assign(words + 1, 0);
  rd->acgt.assign(words + 1, 0);
  rd->woff.assign(nr + 1, 0);
  rd->len.assign(nr, 0);
  if (rfx_pack_spans((const char*)x, so.data(), sl.data(), nullptr, (uint32_t)nr, 0, RFX_PACK_COUNT, rd->codes.data(), rd->acgt.data(),
                     nullptr, rd->woff.data(), rd->len.data()) != RFX_OK) {
    delete rd;
    return nullptr;
  }
  return rd;
}

// the FASTA mode's two: include/rufus_hip.h says what they answer; the statements are rfx_fasta_core.h's
int rfx_text_settle_fasta(rfx_text* t, rfx_text* next, uint64_t* carried) {
  *carried = 0;
  if (next == t || (next && !next->text.empty())) return RFX_E_INVAL;
  if (t->failed) return RFX_E_FORMAT;
  const uint64_t n = t->text.size();
  if (n == 0) return RFX_OK;
  std::vector<uint8_t> copy(t->text);
  if (copy[0] != '>') {
    g_error = "rfx_fasta: the text does not begin with '>'";
    return RFX_E_FORMAT;
  }
  uint64_t cut = n;
  if (next) {
    const std::vector<uint64_t> ls = line_starts(copy.data(), n);
    cut = 0;
    for (size_t i = 1; i < ls.size(); ++i)  // k_fa_last_header
      if (fa_is_header(copy.data(), n, ls[i], n)) cut = std::max(cut, ls[i]);
    if (cut == 0) {
      char msg[160];
      snprintf(msg, sizeof msg, "rfx_fasta: one sequence fills the text arena of %llu bytes", (unsigned long long)n);
      g_error = msg;
      return RFX_E_RANGE;
    }
  }
  const int rc = cut_text(t, next, cut, carried);
  if (rc == RFX_OK) printf("settle %llu %llu\n", (unsigned long long)n, (unsigned long long)*carried);
  return rc;
}
rfx_reads* rfx_text_parse_fasta(rfx_text* t, int flags, int* fasta) {
  *fasta = 1;
  if (t->failed || flags != RFX_PACK_COUNT) return nullptr;
  rfx_reads* rd = new rfx_reads;
  if (!pack_text(t->text.data(), t->text.size(), *rd)) {
    delete rd;
    *fasta = 0;
    return nullptr;
  }
  return rd;
}

}  // extern "C"

static std::vector<uint8_t> read_file(const char* path) {
  std::ifstream f(path, std::ios::binary);
  if (!f.is_open()) rfxcli::die(std::string("cannot open ") + path);
  return std::vector<uint8_t>(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
}

int main(int argc, char** argv) {
  if (argc >= 3 && !strcmp(argv[1], "core")) {
    const bool trunc = !strcmp(argv[2], "--trunc");
    for (int a = trunc ? 3 : 2; a < argc; ++a) {
      const std::vector<uint8_t> text = read_file(argv[a]);
      for (uint64_t n = trunc ? 0 : text.size(); n <= text.size(); ++n) {
        rfx_reads b;
        const bool fasta = pack_text(text.data(), n, b);
        print_block(n, fasta, b);
      }
    }
    return 0;
  }
  if (argc >= 5 && !strcmp(argv[1], "ingest")) {
    const size_t arena = (size_t)atoll(argv[2]), piece = (size_t)atoll(argv[3]);
    rfx_ctx ctx{0};
    std::unique_ptr<rfxcli::BgzfIngest> route[2];  // [1]: the FASTA mode -- every input decides for itself
    for (int a = 4; a < argc; ++a) {
      const std::vector<uint8_t> gz = read_file(argv[a]);
      const int fd = ::open(argv[a], O_RDONLY);
      if (fd < 0) rfxcli::die(std::string("cannot open ") + argv[a]);
      const bool fasta = rfxcli::bgzf_first_byte(fd, gz.size()) == '>';
      ::close(fd);
      if (!route[fasta])
        route[fasta].reset(new rfxcli::BgzfIngest(&ctx, [](rfx_reads* r) { print_reads(*r); rfx_reads_free(r); }, arena, piece, fasta));
      route[fasta]->feed_mapped((const char*)gz.data(), gz.size());
      printf("ok %s\n", route[fasta]->counts().c_str());
    }
    return 0;
  }
  fprintf(stderr, "usage: fasta_harness core [--trunc] FILE... | fasta_harness ingest ARENA_BYTES PIECE_BYTES FILE.gz...\n");
  return 2;
}
