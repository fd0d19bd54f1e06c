// Stand-alone host harness of the lock-step driver of `RUFUS.Filter A.fastq.gz B.fastq.gz` (rufus_amd/csrc/host/
// rfx_ingest.hpp, class BgzfPairFilter): the class as the executable uses it, over HOST stand-ins for the device entry
// points it calls, so that the logic that is easy to get wrong -- two arenas per mate, the cut at the smaller record count,
// the tails that move to the next arena, the ends of the two files -- runs in the CPU suite, plain and under
// -fsanitize=address,undefined (tests/test_filter_bgzf_host.py builds both).  TEST INFRASTRUCTURE: nothing here is built
// into the product, whose RUFUS.Filter has no CPU path.
//   arenas                        byte vectors
//   rfx_text_append_bgzf          the host side of rufus_amd/csrc/rfx_bgzf_core.h (the statements k_bgzf_inflate runs)
//   records / settle_records / gather / parse / rfx_filter      plain C++ over the bytes
// The host half of the library is the real one (rfx_bgzf_scan, rfx_pack_spans, rfx_hashlist_keys): build with
//   g++ -O1 -g -std=c++17 -pthread filter_bgzf_harness.cpp ../../rufus_amd/csrc/rfx_host.cpp
//
//   filter_bgzf_harness HASHLIST A.gz B.gz K MINQ THRESH ARENA_BYTES PIECE_BYTES
// runs the driver, then computes the pulled records DIRECTLY -- both files inflated whole, record i of A beside record i
// of B, the scan of src/RUFUS.Filter.cpp:196-220 on the text of each -- and compares byte for byte.  Prints
//   ok steps <n> pairs <n> pulled <n> bytes1 <n> bytes2 <n>
// and exits 0; a difference exits 3.  What the driver refuses ends the process with its message and exit 1 (die()).
#include <cstdlib>
#include <fstream>
#include <unordered_set>
#include <vector>

#include "../../rufus_amd/csrc/host/rfx_ingest.hpp"
#include "../../rufus_amd/csrc/rfx_bgzf_core.h"

struct rfx_ctx { int device; };
struct rfx_set {
  std::unordered_set<uint64_t> keys;
  int k;
};
struct rfx_reads {
  std::vector<uint64_t> codes;
  std::vector<uint32_t> good, woff, len;
};
struct rfx_text {
  std::vector<uint8_t> text;
  uint64_t cap = 0;
  uint32_t n_blocks = 0;
  bool failed = false;
  long tickets = 0;
};

static std::string g_error = "host stand-in";

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

// one block: BGZF_OK and its bytes, or the core's status
static uint32_t inflate_block(const uint8_t* b, uint32_t pay_off, uint32_t pay_len, uint32_t isize, uint32_t crc, std::vector<uint8_t>& out) {
  static bgzf_tables* tables = new bgzf_tables();
  std::vector<uint8_t> in(b + pay_off, b + pay_off + pay_len);  // (a heap block of exactly the payload's size)
  out.assign(isize, 0);
  SerialOut so{out.data()};
  uint32_t st = bgzf_inflate(in.data(), in.data() + in.size(), isize, *tables, so);
  if (st == BGZF_OK && ~bgzf_crc_update(0xFFFFFFFFu, out.data(), isize) != crc) st = BGZF_E_CRC;
  return st;
}

// the byte behind newline i of text[0, n), i = 1 ..: line_start as the device makes it (ls[0] = 0)
static std::vector<uint64_t> line_starts(const uint8_t* t, uint64_t n) {
  std::vector<uint64_t> ls{0};
  for (uint64_t i = 0; i < n; ++i)
    if (t[i] == '\n') ls.push_back(i + 1);
  return ls;
}

extern "C" {

const char* rfx_last_error(void) { return g_error.c_str(); }
void* rfx_host_alloc(size_t bytes) { return malloc(bytes); }
void rfx_host_free(void* p) { free(p); }

rfx_set* rfx_set_build(rfx_ctx*, const uint64_t* fwd_keys, uint64_t n, int k) {
  rfx_set* s = new rfx_set;
  s->k = k;
  s->keys.insert(fwd_keys, fwd_keys + n);
  return s;
}
void rfx_set_free(rfx_set* s) { delete s; }
void rfx_reads_free(rfx_reads* r) { delete r; }
uint64_t rfx_reads_of_length(const rfx_reads* r, uint32_t len) {
  uint64_t c = 0;
  for (uint32_t l : r->len) c += l == len;
  return c;
}

// (tests/host/filter_sam_harness.cpp's: the loop of src/RUFUS.Filter.cpp:203-220 on the packed arrays)
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
    if (found >= (uint32_t)thresh) {
      ++over;
      if (hitmask_out) hitmask_out[x >> 6] |= 1ull << (x & 63);
    }
  }
  if (n_hit_reads) *n_hit_reads = over;
  return RFX_OK;
}

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
  std::vector<uint8_t> copy((const uint8_t*)host, (const uint8_t*)host + n), out;  // (exactly n bytes: the scan's and the headers' reads)
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
int rfx_text_records(rfx_text* t, uint64_t* records) {
  *records = 0;
  if (t->failed) return RFX_E_FORMAT;
  *records = (line_starts(t->text.data(), t->text.size()).size() - 1) / 4;
  return RFX_OK;
}
int rfx_text_settle_records(rfx_text* t, rfx_text* next, uint64_t max_records, uint64_t* records, uint64_t* carried) {
  *records = *carried = 0;
  if (next == t || (next && !next->text.empty())) return RFX_E_INVAL;
  if (t->failed) return RFX_E_FORMAT;
  const std::vector<uint64_t> ls = line_starts(t->text.data(), t->text.size());
  const uint64_t n = std::min<uint64_t>((ls.size() - 1) / 4, max_records), cut = ls[4 * n], tail = t->text.size() - cut;
  if (tail) {
    if (!next) return RFX_E_FORMAT;
    if (tail > next->cap) return RFX_E_RANGE;
    next->text.assign(t->text.begin() + (long)cut, t->text.end());
  }
  t->text.resize(cut);
  t->text.shrink_to_fit();
  *records = n;
  *carried = tail;
  return RFX_OK;
}
int rfx_text_gather(rfx_text* t, const uint64_t* hitmask, uint64_t n_records, void* host_out, uint64_t cap, uint64_t* bytes,
                    uint64_t* n_selected) {
  *bytes = 0;
  if (n_selected) *n_selected = 0;
  if (t->failed) return RFX_E_FORMAT;
  const std::vector<uint64_t> ls = line_starts(t->text.data(), t->text.size());
  if (ls.size() - 1 != 4 * n_records || ls.back() != t->text.size()) return RFX_E_INVAL;
  uint64_t need = 0, sel = 0;
  for (uint64_t r = 0; r < n_records; ++r)
    if ((hitmask[r >> 6] >> (r & 63)) & 1) {
      need += ls[4 * r + 4] - ls[4 * r];
      ++sel;
    }
  *bytes = need;
  if (n_selected) *n_selected = sel;
  if (need > cap) return RFX_E_RANGE;
  uint8_t* o = (uint8_t*)host_out;
  for (uint64_t r = 0; r < n_records; ++r)
    if ((hitmask[r >> 6] >> (r & 63)) & 1) {
      memcpy(o, t->text.data() + ls[4 * r], ls[4 * r + 4] - ls[4 * r]);
      o += ls[4 * r + 4] - ls[4 * r];
    }
  return RFX_OK;
}
// what rfx_text_parse accepts (rfx_text.hip k_txt_reads), packed by the host packer
rfx_reads* rfx_text_parse(rfx_text* t, int flags, int min_q, int* strict) {
  *strict = 1;
  if (t->failed || flags != RFX_PACK_FILTER) return nullptr;
  const uint8_t* x = t->text.data();
  const uint64_t n = t->text.size();
  const std::vector<uint64_t> ls = line_starts(x, n);
  const uint64_t lines = ls.size() - 1;
  *strict = 0;
  if (n == 0 || x[n - 1] != '\n' || lines == 0 || (lines & 3)) return nullptr;
  const uint64_t nr = lines / 4;
  std::vector<uint64_t> so(nr), qo(nr);
  std::vector<uint32_t> sl(nr);
  uint64_t words = 0;
  for (uint64_t r = 0; r < nr; ++r) {
    const uint64_t l0 = ls[4 * r], l1 = ls[4 * r + 1], l2 = ls[4 * r + 2], l3 = ls[4 * r + 3], l4 = ls[4 * r + 4];
    const uint64_t L = l2 - 1 - l1, Q = l4 - 1 - l3;
    if (!(l1 - l0 >= 2 && x[l0] == '@' && l3 - l2 >= 2 && x[l2] == '+' && L == Q)) return nullptr;
    so[r] = l1;
    qo[r] = l3;
    sl[r] = (uint32_t)L;
    words += (L + 31) / 32;
  }
  *strict = 1;
  rfx_reads* rd = new rfx_reads;
  rd->codes.assign(words + 1, 0);
  rd->good.assign(words + 1, 0);
  rd->woff.assign(nr + 1, 0);
  rd->len.assign(nr, 0);
  if (rfx_pack_spans((const char*)x, so.data(), sl.data(), qo.data(), (uint32_t)nr, min_q, RFX_PACK_FILTER, rd->codes.data(), nullptr,
                     rd->good.data(), rd->woff.data(), rd->len.data()) != RFX_OK) {
    delete rd;
    return nullptr;
  }
  return rd;
}

}  // extern "C"

// ---- the direct computation -------------------------------------------------------------------------------------------
static std::vector<uint8_t> read_file(const char* path) {
  std::ifstream f(path, std::ios::binary);
  if (!f.is_open()) rfxcli::die(std::string("cannot open ") + path);
  return std::vector<uint8_t>(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
}

static std::vector<uint8_t> inflate_whole(const std::vector<uint8_t>& gz) {
  std::vector<uint8_t> text, out;
  for (uint64_t at = 0; at < gz.size();) {
    uint32_t bsize, pay_off, pay_len, isize, crc;
    if (bgzf_block_header(gz.data() + at, gz.size() - at, &bsize, &pay_off, &pay_len, &isize, &crc) != 0) rfxcli::die("direct: not BGZF");
    if (inflate_block(gz.data() + at, pay_off, pay_len, isize, crc, out) != BGZF_OK) rfxcli::die("direct: a block does not inflate");
    text.insert(text.end(), out.begin(), out.end());
    at += bsize;
  }
  if (!text.empty() && text.back() != '\n') text.push_back('\n');
  return text;
}

// src/RUFUS.Filter.cpp:196-220 on one record's sequence and quality line
static bool hit(const rfx_set& s, const uint8_t* seq, const uint8_t* qual, uint64_t L, int min_q, int thresh) {
  const uint64_t kmask = s.k >= 32 ? ~0ull : (1ull << (2 * s.k)) - 1;
  uint64_t key = 0;
  int streak = 0, found = 0;
  for (uint64_t i = 0; i + 1 < L; ++i) {
    const uint8_t ch = seq[i];
    const uint64_t code = ch == 'C' ? 1 : ch == 'G' ? 2 : ch == 'T' ? 3 : 0;
    const bool good = !((int)(signed char)qual[i] - 33 < min_q || ch == 'N');
    key = ((key << 2) | code) & kmask;
    streak = good ? streak + 1 : 0;
    if (streak >= s.k && s.keys.count(key)) ++found;
  }
  return found >= thresh;
}

int main(int argc, char** argv) {
  if (argc < 9) {
    fprintf(stderr, "usage: filter_bgzf_harness HASHLIST A.gz B.gz K MINQ THRESH ARENA_BYTES PIECE_BYTES\n");
    return 2;
  }
  const int k = atoi(argv[4]), min_q = atoi(argv[5]), thresh = atoi(argv[6]);
  const size_t arena = (size_t)atoll(argv[7]), piece = (size_t)atoll(argv[8]);
  const std::vector<uint8_t> hl = read_file(argv[1]), gz1 = read_file(argv[2]), gz2 = read_file(argv[3]);
  const long nk = rfx_hashlist_keys((const char*)hl.data(), hl.size(), k, 0, nullptr, 0);
  if (nk < 0) rfxcli::die("cannot parse the hash list");
  std::vector<uint64_t> keys((size_t)nk + 1);
  rfx_hashlist_keys((const char*)hl.data(), hl.size(), k, 0, keys.data(), keys.size());
  rfx_ctx ctx{0};
  rfx_set* set = rfx_set_build(&ctx, keys.data(), (uint64_t)nk, k);
  std::string got1, got2;
  uint64_t pairs = 0, pulled = 0;
  std::string counts;
  {
    rfxcli::BgzfPairFilter route(
        &ctx, set, min_q, thresh,
        [&](const char* a, size_t na, const char* b, size_t nb, uint64_t p, uint64_t f) {
          got1.append(a, na);
          got2.append(b, nb);
          pairs += p;
          pulled += f;
        },
        arena, piece);
    route.run((const char*)gz1.data(), gz1.size(), (const char*)gz2.data(), gz2.size());
    counts = route.counts();
  }
  // directly
  const std::vector<uint8_t> t1 = inflate_whole(gz1), t2 = inflate_whole(gz2);
  const std::vector<uint64_t> l1 = line_starts(t1.data(), t1.size()), l2 = line_starts(t2.data(), t2.size());
  const uint64_t n1 = (l1.size() - 1) / 4, n2 = (l2.size() - 1) / 4;
  if (n2 < n1) {
    fprintf(stderr, "direct: mate 2 is short, and the driver did not refuse it\n");
    return 3;
  }
  std::string want1, want2;
  uint64_t want_pulled = 0;
  for (uint64_t r = 0; r < n1; ++r) {
    const bool h1 = hit(*set, t1.data() + l1[4 * r + 1], t1.data() + l1[4 * r + 3], l1[4 * r + 2] - 1 - l1[4 * r + 1], min_q, thresh);
    const bool h2 = hit(*set, t2.data() + l2[4 * r + 1], t2.data() + l2[4 * r + 3], l2[4 * r + 2] - 1 - l2[4 * r + 1], min_q, thresh);
    if (h1 || h2) {
      want1.append((const char*)t1.data() + l1[4 * r], l1[4 * r + 4] - l1[4 * r]);
      want2.append((const char*)t2.data() + l2[4 * r], l2[4 * r + 4] - l2[4 * r]);
      ++want_pulled;
    }
  }
  if (pairs != n1 || pulled != want_pulled || got1 != want1 || got2 != want2) {
    fprintf(stderr, "MISMATCH: pairs %llu (direct %llu), pulled %llu (direct %llu), bytes %zu / %zu (direct %zu / %zu)\n",
            (unsigned long long)pairs, (unsigned long long)n1, (unsigned long long)pulled, (unsigned long long)want_pulled, got1.size(),
            got2.size(), want1.size(), want2.size());
    return 3;
  }
  // "filter: bgzf route: B blocks in A appends, S steps, ..."
  unsigned long long blocks = 0, appends = 0, steps = 0;
  sscanf(counts.c_str(), "filter: bgzf route: %llu blocks in %llu appends, %llu steps", &blocks, &appends, &steps);
  printf("ok steps %llu pairs %llu pulled %llu bytes1 %zu bytes2 %zu\n", steps, (unsigned long long)pairs, (unsigned long long)pulled,
         got1.size(), got2.size());
  if (argc > 9) {  // the pulled records, for the caller's own comparison
    std::ofstream(std::string(argv[9]) + ".Mate1.fastq", std::ios::binary).write(got1.data(), (std::streamsize)got1.size());
    std::ofstream(std::string(argv[9]) + ".Mate2.fastq", std::ios::binary).write(got2.data(), (std::streamsize)got2.size());
  }
  rfx_set_free(set);
  return 0;
}
