// Parallel FASTQ ingest of the drop-in `jellyfish count`: text in, packed read blocks in HBM out.
//
// The reference parses with one producer per file (jf/include/jellyfish/mer_overlap_sequence_parser.hpp:
// 124-251) and hashes in T threads.  Here the device counts ~100x faster than one core can parse, so the host
// side is the pipeline to get right:
//
//   regular file   mmap; the byte range is cut into ~32 MB pieces at record boundaries, every worker parses
//                  and packs pieces on its own (no reader thread in the way)
//   pipe / FIFO    one reader thread (the stream cannot be split) cuts the byte stream every 4k lines and hands
//                  the pieces to the workers
//   workers        find the sequence lines of their piece, reserve a range of the current staging block (pinned
//                  host memory: 2-bit codes, ACGT mask, offsets, lengths) and pack straight into it
//                  (rfx_pack_spans) -- no intermediate copy of the text
//   main thread    uploads every full block (rfx_reads_upload) and hands it to the caller (count it, or keep it
//                  for the shard passes of rfx_count_set_passes)
//
// Only strict 4-line FASTQ takes this path (what PassThroughSamCheck and every sequencer write); FASTA and
// multi-line FASTQ go through the sequential parser of rfx_cli.hpp, which follows the reference's grammar.
#pragma once
#include <sys/mman.h>
#include <sys/stat.h>

#include <atomic>
#include <chrono>
#include <condition_variable>
#include <deque>
#include <functional>
#include <limits>
#include <map>
#include <memory>
#include <mutex>
#include <thread>

#include "rfx_cli.hpp"

#include "rfx_sam.hpp"
#include "rfx_bam_pairs.hpp"
#include "rfx_bam_single.hpp"
#include "rfx_packed_cache.hpp"
#include "rfx_bam_cache.hpp"
#include "rfx_bai.hpp"
#include "../rfx_bgzf_core.h"
#include "../rfx_gzip_core.h"

namespace rfxcli {

// pread until `want` bytes are there, the file ends or a read fails (EINTR: again).  Returns the bytes read; errno is the
// failed read's.
inline size_t pread_all(int fd, void* buf, size_t want, uint64_t off) {
  size_t got = 0;
  while (got < want) {
    const ssize_t n = ::pread(fd, (char*)buf + got, want - got, (off_t)(off + got));
    if (n < 0 && errno == EINTR) continue;
    if (n <= 0) break;
    got += (size_t)n;
  }
  return got;
}
// The first min(size, cap) bytes of an open regular file, or as many of them as can be read: what the routes sniff.
inline std::vector<uint8_t> read_head(int fd, uint64_t size, size_t cap) {
  std::vector<uint8_t> head((size_t)std::min<uint64_t>(size, cap));
  head.resize(pread_all(fd, head.data(), head.size(), 0));
  return head;
}

// The stream cutter's line count. Fast pass: newlines of [p, e) and how many of them are blank lines (a '\n' at a
// line start); at_start (in / out): the byte at p begins a line.
static inline void count_newlines_plain(const char* p, const char* e, bool& at_start, size_t& nl, size_t& blanks) {
  for (; p < e; ++p) {
    if (*p == '\n') {
      ++nl;
      blanks += at_start;
      at_start = true;
    } else {
      at_start = false;
    }
  }
}
#if RFX_X86
__attribute__((target("avx2,popcnt"))) static inline void count_newlines_avx2(const char* p, const char* e, bool& at_start,
                                                                             size_t& nl, size_t& blanks) {
  const __m256i v = _mm256_set1_epi8('\n');
  while (e - p >= 32) {
    const uint32_t m = (uint32_t)_mm256_movemask_epi8(_mm256_cmpeq_epi8(_mm256_loadu_si256((const __m256i*)p), v));
    nl += (size_t)__builtin_popcount(m);
    blanks += (size_t)__builtin_popcount(m & ((m << 1) | (at_start ? 1u : 0u)));
    at_start = (m >> 31) & 1u;
    p += 32;
  }
  count_newlines_plain(p, e, at_start, nl, blanks);
}
#endif
static inline void count_newlines(const char* p, const char* e, bool& at_start, size_t& nl, size_t& blanks) {
  nl = blanks = 0;
#if RFX_X86
  static const bool fast = (__builtin_cpu_init(), __builtin_cpu_supports("avx2") && __builtin_cpu_supports("popcnt"));
  if (fast) return count_newlines_avx2(p, e, at_start, nl, blanks);
#endif
  count_newlines_plain(p, e, at_start, nl, blanks);
}
// Slow pass (only for stretches that hold blank lines): the grammar parse_piece applies -- blank lines BETWEEN records
// are skipped, an empty sequence or quality line inside a record is a line.  line_in_rec: lines of the current
// record seen so far; rec_end: set to just after the last line that completed a record (untouched if none did).
static inline void walk_fastq_lines(const char* p, const char* e, bool& at_start, uint64_t& line_in_rec, const char*& rec_end) {
  bool partial = !at_start;  // p continues a line that began earlier: it is not blank
  while (p < e) {
    const char* nl = (const char*)memchr(p, '\n', (size_t)(e - p));
    if (!nl) {
      at_start = false;
      return;
    }
    const bool blank = nl == p && !partial;
    partial = false;
    if (!(line_in_rec == 0 && blank) && ++line_in_rec == 4) {
      line_in_rec = 0;
      rec_end = nl + 1;
    }
    p = nl + 1;
    at_start = true;
  }
}

struct StageBlock {
  uint64_t* codes = nullptr;
  uint32_t *acgt = nullptr, *word_off = nullptr, *len = nullptr;
  bool pinned = true;  // false: made by a lazy allocator (no call into the device runtime), page-locked before its first upload
  uint32_t cap_reads = 0, n_reads = 0;
  uint64_t cap_words = 0, n_words = 0;
  int writers = 0;
  bool sealed = false;
};

class CountIngest {
  std::function<void(const StageBlock&)> sink_;
  unsigned nthreads_;
  void (*dealloc_)(void*);
  int (*pin_)(void*) = nullptr;  // late page-locking of the staging blocks (rfx_host_alloc_lazy + rfx_host_pin)
  void pin_block(StageBlock& b) {
    if (b.pinned || !pin_) return;
    (void)pin_(b.codes); (void)pin_(b.acgt); (void)pin_(b.word_off); (void)pin_(b.len);  // (a refusal: the upload is staged by the runtime)
    b.pinned = true;
  }
  std::vector<StageBlock> blocks_;
  std::mutex mu_;
  std::condition_variable cv_;  // one for every state change: pieces, blocks, failure
  struct Piece {
    const char* b;
    const char* e;
    std::vector<char>* owner;  // heap buffer of a pipe piece (returned to the pool), null otherwise
    int fd = -1;               // >= 0: a byte range [lo, hi) of a regular file -- the worker reads it itself and
    uint64_t lo = 0, hi = 0;   // parses the records that START inside the range
    uint64_t fsize = 0;
    uint64_t seq = 0;          // SAM mode: position of the piece in the stream (the chromosome log is stitched in order)
    uint64_t spool_off = 0;    // set_spool: where the piece's bytes go in the spool file
  };
  uint64_t stream_bytes_ = 0;  // feed_stream: bytes read so far
  int spool_fd_ = -1;          // set_spool: the stream is also written to this file, piece by piece, by the workers
  uint64_t spooled_ = 0;
  // set_keep_packed (`jellyfish count --sam .. --keep-packed FILE`): every SAM piece also leaves a chunk
  // of the packed-read cache `RUFUS.Filter --packed` scans (rfx_packed_cache.hpp) -- the records as the filter would
  // see them, packed once, here, by the threads that parse the text anyway
  int cache_fd_ = -1, cache_minq_ = 0;
  std::atomic<uint64_t> cache_at_{0};
  std::deque<Piece> work_;
  std::deque<int> ready_, free_;
  std::deque<std::vector<char>*> pool_;
  int current_ = -1;
  bool closing_ = false;
  size_t pieces_open_ = 0;
  std::atomic<bool> drop_mapped_{false};  // pieces without an owner are ranges of a file mapping (feed_mapped)
  std::atomic<bool> failed_{false};
  std::string fail_msg_;
  std::vector<std::thread> workers_;
  std::thread pinner_;
  uint64_t reads_total_ = 0;

  size_t PIECE = 32u << 20;  // bytes of text per piece (tests shrink it)
  // SAM mode (`jellyfish count --sam`): one record per line, the sequence is field 10; the runs of equal RNAME
  // (field 3) of every piece are kept, in stream order they are PassThroughSamCheck's chromosome log
  // (src/PassThroughSamCheck.cpp:140-155)
  bool sam_ = false;
  uint64_t next_seq_ = 0;
  std::map<uint64_t, std::vector<std::string>> chr_runs_;
  const skip_lines_fn skip_lines_ = pick_skip_lines();

  void fail(const std::string& m) {
    std::lock_guard<std::mutex> g(mu_);
    if (!failed_.exchange(true)) fail_msg_ = m;
    cv_.notify_all();
  }

  // Reserve n reads / w words in the current block (sealing it and taking a fresh one when they do not fit).
  bool reserve(uint32_t n, uint64_t w, int& blk, uint32_t& r0, uint64_t& w0) {
    std::unique_lock<std::mutex> g(mu_);
    for (;;) {
      if (failed_) return false;
      if (current_ >= 0) {
        StageBlock& b = blocks_[(size_t)current_];
        if (b.n_reads + (uint64_t)n <= b.cap_reads && b.n_words + w <= b.cap_words) {
          blk = current_;
          r0 = b.n_reads;
          w0 = b.n_words;
          b.n_reads += n;
          b.n_words += w;
          ++b.writers;
          return true;
        }
        b.sealed = true;
        if (b.writers == 0) {
          ready_.push_back(current_);
          cv_.notify_all();
        }
        current_ = -1;
      }
      if (n > blocks_[0].cap_reads || w > blocks_[0].cap_words) {
        g.unlock();
        fail("a read is longer than a staging block");
        return false;
      }
      // (another worker may install the next block while this one waits: look again before taking one)
      cv_.wait(g, [&] { return current_ >= 0 || !free_.empty() || failed_; });
      if (failed_) return false;
      if (current_ >= 0) continue;
      current_ = free_.front();
      free_.pop_front();
      StageBlock& b = blocks_[(size_t)current_];
      b.n_reads = 0;
      b.n_words = 0;
      b.writers = 0;
      b.sealed = false;
      cv_.notify_all();
    }
  }

  void release(int blk) {
    std::lock_guard<std::mutex> g(mu_);
    StageBlock& b = blocks_[(size_t)blk];
    if (--b.writers == 0 && b.sealed) {
      ready_.push_back(blk);
      cv_.notify_all();
    }
  }

  void parse_piece(const Piece& pc) {
    std::vector<uint64_t> start;
    std::vector<uint32_t> slen;
    start.reserve(1 << 17);
    slen.reserve(1 << 17);
    const char *p = pc.b, *e = pc.e;
    uint64_t words = 0;
    while (p < e) {
      if (*p == '\n') { ++p; continue; }  // blank lines between records are skipped (as the reference's parser does)
      if (*p != '@') return fail("parallel FASTQ reader: a record does not start with '@' (multi-line FASTQ? use RFX_HOST_THREADS=1)");
      const char* nl = find_nl(p, e);
      if (!nl) return fail("truncated FASTQ record");
      const char* s = nl + 1;
      nl = find_nl(s, e);
      if (!nl) return fail("truncated FASTQ record");
      const size_t L = (size_t)(nl - s);
      const char* plus = nl + 1;
      if (plus >= e || *plus != '+') return fail("parallel FASTQ reader: multi-line FASTQ records (use RFX_HOST_THREADS=1)");
      nl = plus + 1 < e && plus[1] == '\n' ? plus + 1 : find_nl(plus, e);  // almost always a bare "+"
      if (!nl) return fail("truncated FASTQ record");
      const char* q = nl + 1;
      // the quality line has to be as long as the sequence: look there first, search only if that is not its end
      const char* qe = (size_t)(e - q) > L && q[L] == '\n' && !memchr(q, '\n', L) ? q + L : find_nl(q, e);
      if (!qe) qe = e;  // last record of a file without a final newline
      if ((size_t)(qe - q) != L) return fail("parallel FASTQ reader: quality and sequence lengths differ (multi-line FASTQ? use RFX_HOST_THREADS=1)");
      start.push_back((uint64_t)(s - pc.b));
      slen.push_back((uint32_t)L);
      words += (L + 31) / 32;
      p = qe < e ? qe + 1 : e;
    }
    pack_spans_of(pc, start, slen);
    (void)words;
  }

  // SAM text (no header lines: `samtools view` without -h, as scripts/RunJellyForRUFUS.sh feeds it): what
  // PassThroughSamCheck would print as the sequence line of each record, packed in place.
  void parse_piece_sam(const Piece& pc) {
    std::vector<uint64_t> start;
    std::vector<uint32_t> slen;
    start.reserve(1 << 17);
    slen.reserve(1 << 17);
    std::vector<std::string> runs, cache_runs;
    rfxcache::ChunkBuilder cache;
    const char *p = pc.b, *e = pc.e;
    const char *cur_chr = nullptr, *cache_chr = nullptr;
    size_t cur_len = 0, cache_chr_len = 0;
    while (p < e) {
      const char* nl = find_nl(p, e);
      const char* le = nl ? nl : e;
      // tabs 2 and 3 bound RNAME, tabs 9 and 10 (or the end of the line) bound SEQ
      const char* tab[10];
      int nt = 0;
      for (const char* q = p; nt < 10 && q < le;) {
        const char* t = (const char*)memchr(q, '\t', (size_t)(le - q));
        if (!t) break;
        tab[nt++] = t;
        q = t + 1;
      }
      if (nt < 9) return fail("--sam: a line has fewer than 10 tab-separated fields (a header? feed `samtools view` without -h)");
      const char* chr = tab[1] + 1;
      const size_t chr_len = (size_t)(tab[2] - chr);
      if (!cur_chr || chr_len != cur_len || memcmp(chr, cur_chr, chr_len) != 0) {
        runs.emplace_back(chr, chr_len);
        cur_chr = chr;
        cur_len = chr_len;
      }
      const char* sq = tab[8] + 1;
      const char* sq_e = nt >= 10 ? tab[9] : le;
      start.push_back((uint64_t)(sq - pc.b));
      slen.push_back((uint32_t)(sq_e - sq));
      if (cache_fd_ >= 0 && nt >= 10) {  // (fewer than 11 fields: no record for the filter -- the feeders skip the line)
        // the filter's chromosome log lists the lines it is given (rufus_filter_main.cpp, split_sam): the cache keeps
        // runs of its own, of these lines only
        if (!cache_chr || chr_len != cache_chr_len || memcmp(chr, cache_chr, chr_len) != 0) {
          cache_runs.emplace_back(chr, chr_len);
          cache_chr = chr;
          cache_chr_len = chr_len;
        }
        const char* ql = tab[9] + 1;
        const char* ql_e = (const char*)memchr(ql, '\t', (size_t)(le - ql));
        if (!ql_e) ql_e = le;
        cache.add(pc.b, p, le, p, tab[0], tab[0] + 1, tab[1], sq, sq_e, ql, ql_e);
      }
      p = nl ? nl + 1 : e;
    }
    if (cache_fd_ >= 0) {
      std::vector<char> chunk;
      cache.finish(pc.seq, pc.spool_off, cache_runs, cache_minq_, chunk);
      const uint64_t at = cache_at_.fetch_add(chunk.size());
      const char* w = chunk.data();
      size_t len = chunk.size();
      off_t o = (off_t)at;
      while (len) {
        const ssize_t n = ::pwrite(cache_fd_, w, len, o);
        if (n < 0 && errno == EINTR) continue;
        if (n <= 0) die(std::string("write error on the packed-read cache: ") + strerror(errno));
        w += n;
        len -= (size_t)n;
        o += n;
      }
    }
    {
      std::lock_guard<std::mutex> g(mu_);
      chr_runs_[pc.seq] = std::move(runs);
    }
    pack_spans_of(pc, start, slen);
  }

  void pack_spans_of(const Piece& pc, const std::vector<uint64_t>& start, const std::vector<uint32_t>& slen) {
    // normally one reservation per piece; a piece with more reads than a staging block holds goes in slices
    const size_t total = start.size();
    size_t at = 0;
    std::vector<uint32_t> woff_tmp;
    while (at < total) {
      uint32_t n = 0;
      uint64_t w = 0;
      while (at + n < total && n < blocks_[0].cap_reads / 2 + 1) {
        const uint64_t wr = (slen[at + n] + 31) / 32;
        if (n && w + wr > blocks_[0].cap_words / 2) break;
        w += wr;
        ++n;
      }
      int blk;
      uint32_t r0;
      uint64_t w0;
      if (!reserve(n, w, blk, r0, w0)) return;
      StageBlock& b = blocks_[(size_t)blk];
      // rfx_pack_spans writes n + 1 offsets, the last one being the neighbour range's first: it gets an array of this
      // thread's own, and only the range's n entries go into the block (two threads storing the same value into one
      // entry is still a data race -- ThreadSanitizer, tests/test_tsan_host.py); the entry behind the block's last
      // read is the consumer's to write
      woff_tmp.resize((size_t)n + 1);
      woff_tmp[0] = (uint32_t)w0;
      const int rc = rfx_pack_spans(pc.b, start.data() + at, slen.data() + at, nullptr, n, 0, RFX_PACK_COUNT, b.codes, b.acgt,
                                    nullptr, woff_tmp.data(), b.len + r0);
      if (rc) fail(std::string("rfx_pack_spans: ") + rfx_strerror(rc));
      memcpy(b.word_off + r0, woff_tmp.data(), (size_t)n * sizeof(uint32_t));
      release(blk);
      at += n;
    }
  }

  // A range of a regular file: read it (plus one byte before and the tail of the record that straddles its
  // end) into the worker's own buffer -- pread scales with the threads, faulting a 20 GB mapping page by page
  // does not -- and parse the records that start inside [lo, hi).
  void parse_range(const Piece& pc, std::vector<char>& buf) {
    const uint64_t SLACK = 1u << 20;  // longest record the tail may hold
    const uint64_t from = pc.lo ? pc.lo - 1 : 0, to = std::min<uint64_t>(pc.fsize, pc.hi + SLACK);
    buf.resize((size_t)(to - from));
    if (pread_all(pc.fd, buf.data(), buf.size(), from) != buf.size()) return fail(std::string("read error on input: ") + strerror(errno));
    const char *b = buf.data(), *e = buf.data() + buf.size();
    const char* s0 = pc.lo ? record_start(b + 1, b, e) : b;                       // first record starting at >= lo
    const char* hi_p = b + (pc.hi - from);
    const char* s1 = pc.hi >= pc.fsize ? e : record_start(hi_p, b, e);             // first record starting at >= hi
    if (pc.hi < pc.fsize && s1 == e && to < pc.fsize) return fail("a FASTQ record is longer than 1 MB");
    if (s0 >= s1) return;
    parse_piece(Piece{s0, s1, nullptr});
  }

  void worker() {
    std::vector<char> buf;
    for (;;) {
      Piece pc;
      {
        std::unique_lock<std::mutex> g(mu_);
        cv_.wait(g, [&] { return !work_.empty() || closing_ || failed_; });
        if (failed_ || (work_.empty() && closing_)) return;
        pc = work_.front();
        work_.pop_front();
      }
      if (pc.fd >= 0) parse_range(pc, buf);
      else if (sam_) parse_piece_sam(pc);
      else parse_piece(pc);
      if (pc.fd < 0 && !pc.owner && drop_mapped_) drop_mapped(pc.b, pc.e);  // a piece of feed_mapped()'s mapping
      if (spool_fd_ >= 0 && pc.fd < 0 && pc.owner) {  // a piece of a pipe: its bytes, at their place in the stream
        const char* p = pc.b;
        size_t len = (size_t)(pc.e - pc.b);
        off_t at = (off_t)pc.spool_off;
        while (len) {
          const ssize_t w = ::pwrite(spool_fd_, p, len, at);
          if (w < 0 && errno == EINTR) continue;
          if (w <= 0) die(std::string("write error on the spool file: ") + strerror(errno));
          p += w;
          len -= (size_t)w;
          at += w;
        }
      }
      {
        std::lock_guard<std::mutex> g(mu_);
        if (pc.owner) pool_.push_back(pc.owner);
        --pieces_open_;
        cv_.notify_all();
      }
    }
  }

  void push_piece(const Piece& pc) {
    std::lock_guard<std::mutex> g(mu_);
    work_.push_back(pc);
    ++pieces_open_;
    cv_.notify_all();
  }

  // Upload every block that is ready; with `all`, wait until every queued piece is packed and seal the last block.
  void drain(bool all) {
    for (;;) {
      int blk = -1;
      {
        std::unique_lock<std::mutex> g(mu_);
        if (all) {
          cv_.wait(g, [&] { return !ready_.empty() || pieces_open_ == 0 || failed_; });
          if (failed_) break;
          if (ready_.empty() && pieces_open_ == 0) {
            if (current_ >= 0) {  // the partly filled last block
              blocks_[(size_t)current_].sealed = true;
              ready_.push_back(current_);
              current_ = -1;
            } else {
              break;
            }
          }
        }
        if (ready_.empty()) break;
        blk = ready_.front();
        ready_.pop_front();
      }
      StageBlock& b = blocks_[(size_t)blk];
      if (b.n_reads) {
        b.word_off[b.n_reads] = (uint32_t)b.n_words;
        reads_total_ += b.n_reads;
        pin_block(b);
        sink_(b);  // uploads it (rfx_reads_upload): the block is reused as soon as this returns
      }
      {
        std::lock_guard<std::mutex> g(mu_);
        free_.push_back(blk);
        cv_.notify_all();
      }
    }
    if (failed_) die("rufus_amd jellyfish: " + fail_msg_);
  }

  friend class TextIngest;
  // First position >= p where a 4-line FASTQ record starts ('@' line whose third line starts with '+' and whose
  // second and fourth lines are equally long); e when there is none.
  static const char* record_start(const char* p, const char* b, const char* e) {
    if (p <= b) return b;
    const char* nl = (const char*)memchr(p - 1, '\n', (size_t)(e - (p - 1)));
    if (!nl) return e;
    const char* l0 = nl + 1;
    for (int tries = 0; tries < 8 && l0 < e; ++tries) {
      const char* n0 = (const char*)memchr(l0, '\n', (size_t)(e - l0));
      if (!n0) return e;
      const char* l1 = n0 + 1;
      const char* n1 = l1 < e ? (const char*)memchr(l1, '\n', (size_t)(e - l1)) : nullptr;
      const char* l2 = n1 ? n1 + 1 : e;
      const char* n2 = l2 < e ? (const char*)memchr(l2, '\n', (size_t)(e - l2)) : nullptr;
      const char* l3 = n2 ? n2 + 1 : e;
      const char* n3 = l3 < e ? (const char*)memchr(l3, '\n', (size_t)(e - l3)) : nullptr;
      const char* l3e = n3 ? n3 : e;
      if (*l0 == '@' && n1 && n2 && *l2 == '+' && (n1 - l1) == (l3e - l3)) return l0;
      l0 = l1;
    }
    return e;
  }

 public:
  // alloc / dealloc: page-locked memory on the GPU box (rfx_host_alloc), plain malloc in host-only tests
  // pin != nullptr: `alloc` makes plain memory without touching the device runtime (rfx_host_alloc_lazy) -- the workers
  // parse into it while another thread is still opening the device -- and `pin` page-locks a block before its first upload
  CountIngest(unsigned threads, std::function<void(const StageBlock&)> sink, void* (*alloc)(size_t) = rfx_host_alloc,
              void (*dealloc)(void*) = rfx_host_free, uint32_t cap_reads = 4u << 20, uint64_t cap_words = 24ull << 20,
              int (*pin_fn)(void*) = nullptr)
      : sink_(std::move(sink)), nthreads_(threads ? threads : 1), dealloc_(dealloc), pin_(pin_fn) {
    blocks_.resize(3);
    for (StageBlock& b : blocks_) {
      b.cap_reads = cap_reads;
      b.cap_words = cap_words;
      b.pinned = pin_fn == nullptr;
    }
    // Page-locking ~1 GB takes 0.2 s: the workers start on the first block while the others are still being pinned.
    auto pin = [this, alloc](size_t i) {
      StageBlock& b = blocks_[i];
      b.codes = (uint64_t*)alloc(b.cap_words * 8);
      b.acgt = (uint32_t*)alloc(b.cap_words * 4);
      b.word_off = (uint32_t*)alloc(((size_t)b.cap_reads + 1) * 4);
      b.len = (uint32_t*)alloc((size_t)b.cap_reads * 4);
      if (!b.codes || !b.acgt || !b.word_off || !b.len) die("rufus_amd: cannot allocate pinned staging memory");
      std::lock_guard<std::mutex> g(mu_);
      free_.push_back((int)i);
      cv_.notify_all();
    };
    pin(0);
    pinner_ = std::thread([this, pin] {
      for (size_t i = 1; i < blocks_.size(); ++i) pin(i);
    });
    for (unsigned t = 0; t < nthreads_; ++t) workers_.emplace_back([this] { worker(); });
  }

  // The staging memory cut into page-locked pieces of `piece` bytes, for a caller that is done feeding (the count
  // tool drains its result through them).  Valid until this object is destroyed.
  std::vector<std::pair<char*, size_t>> lend_buffers(size_t piece) {
    if (pinner_.joinable()) pinner_.join();
    std::vector<std::pair<char*, size_t>> out;
    for (StageBlock& b : blocks_) {
      pin_block(b);
      for (size_t at = 0; at + piece <= b.cap_words * 8; at += piece) out.emplace_back((char*)b.codes + at, piece);
      for (size_t at = 0; at + piece <= b.cap_words * 4; at += piece) out.emplace_back((char*)b.acgt + at, piece);
    }
    return out;
  }

  ~CountIngest() {
    if (pinner_.joinable()) pinner_.join();
    {
      std::lock_guard<std::mutex> g(mu_);
      closing_ = true;
      cv_.notify_all();
    }
    for (auto& t : workers_) t.join();
    for (auto& b : blocks_) {
      dealloc_(b.codes);
      dealloc_(b.acgt);
      dealloc_(b.word_off);
      dealloc_(b.len);
    }
    for (auto* v : pool_) delete v;
  }

  uint64_t reads() const { return reads_total_; }
  void set_piece_bytes(size_t n) { PIECE = n; }

  // Does the stream look like strict 4-line FASTQ?  (head: its first bytes)
  static bool looks_4line(const char* head, size_t n) {
    if (n == 0 || head[0] != '@') return false;
    const char* e = head + n;
    const char* r = record_start(head, head, e);
    if (r != head) return false;
    // the second record (when the head is long enough to hold it) must follow immediately
    const char* p = head;
    for (int i = 0; i < 4; ++i) {
      const char* nl = (const char*)memchr(p, '\n', (size_t)(e - p));
      if (!nl) return true;
      p = nl + 1;
    }
    return p >= e || *p == '@' || *p == '\n';
  }

  // A whole regular file, mapped.  Returns false if it is not strict 4-line FASTQ (nothing consumed).
  void set_sam(bool on) { sam_ = on; }
  // The bytes of a PIPE input are also written to `fd` (a regular file), so that the stage that reads the same stream
  // next -- RUFUS.Filter after the subject's count, runRufus.sh:966 after scripts/RunJellyForRUFUS.sh:28 -- need not run
  // the generator (samtools view of a BAM) a second time.  Written piece by piece by the parser threads (pwrite).
  void set_spool(int fd) { spool_fd_ = fd; }
  // feed_stream(): called by the reading thread with the number of bytes the stream has delivered so far
  std::function<void(uint64_t)> on_stream_bytes;
  void set_keep_packed(int fd, int min_q) {
    cache_fd_ = fd;
    cache_minq_ = min_q;
    rfxcache::FileHeader h;
    h.min_q = min_q;
    if (::pwrite(fd, &h, sizeof h, 0) != (ssize_t)sizeof h) die("write error on the packed-read cache");
    cache_at_ = sizeof h;
  }
  // after the last feed_*(): the header once more, now with what makes the file a cache (rfx_packed_cache.hpp)
  void finish_keep_packed(uint64_t stream_bytes) {
    if (cache_fd_ < 0) return;
    rfxcache::FileHeader h;
    h.min_q = cache_minq_;
    h.n_chunks = next_seq_;
    h.stream_bytes = stream_bytes;
    h.done = rfxcache::DONE_MAGIC;
    if (::pwrite(cache_fd_, &h, sizeof h, 0) != (ssize_t)sizeof h || ::close(cache_fd_) != 0)
      die(std::string("write error on the packed-read cache: ") + strerror(errno));
    cache_fd_ = -1;
  }
  uint64_t spooled_bytes() const { return spooled_; }
  // PassThroughSamCheck's side file: "notachr", then the name of every run of equal RNAME, in stream order
  std::vector<std::string> chr_log() {
    std::vector<std::string> out{"notachr"};
    for (auto& kv : chr_runs_)
      for (auto& name : kv.second)
        if (out.size() == 1 || out.back() != name) out.push_back(name);
    return out;
  }

  // `data` must be a read-only FILE mapping: the workers drop the page-table entries of what they have parsed
  // (rfx_cli.hpp drop_mapped -- on anonymous memory that would zero it).
  bool feed_mapped(const char* data, size_t size) {
    if (!sam_ && !looks_4line(data, std::min<size_t>(size, 1u << 16))) return false;
    drop_mapped_ = true;
    const char *b = data, *e = data + size;
    const char* at = b;
    while (at < e) {
      const char* want = at + PIECE;
      const char* cut;
      if (want >= e) cut = e;
      else if (sam_) {
        const char* nl = (const char*)memchr(want, '\n', (size_t)(e - want));
        cut = nl ? nl + 1 : e;
      } else cut = record_start(want, b, e);
      Piece pc{at, cut, nullptr};
      pc.seq = next_seq_++;
      pc.spool_off = (uint64_t)(at - b);  // (a regular file is its own spool)
      push_piece(pc);
      at = cut;
      drain(false);
    }
    drain(true);
    return true;
  }

  // A whole regular file by descriptor: byte ranges, read by the workers themselves.  Returns false if the file
  // does not start like strict 4-line FASTQ (nothing consumed).
  bool feed_file(int fd, uint64_t size) {
    const std::vector<uint8_t> head = read_head(fd, size, 1u << 16);
    if (!looks_4line((const char*)head.data(), head.size())) return false;
    for (uint64_t lo = 0; lo < size; lo += PIECE) {
      Piece pc{nullptr, nullptr, nullptr};
      pc.fd = fd;
      pc.lo = lo;
      pc.hi = std::min<uint64_t>(size, lo + PIECE);
      pc.fsize = size;
      push_piece(pc);
      drain(false);
    }
    drain(true);
    return true;
  }

  // A pipe: `head` = bytes already read from it (at least the sniffed prefix).  One reader (this thread) cuts the
  // stream every 4k lines.  Returns false if the head is not strict 4-line FASTQ (the caller then parses
  // head + rest sequentially).
  bool feed_stream(int fd, std::vector<char>& head) {
    if (!sam_ && !looks_4line(head.data(), head.size())) return false;
    const uint64_t lines_per_rec = sam_ ? 1 : 4;
#ifdef F_SETPIPE_SZ
    (void)fcntl(fd, F_SETPIPE_SZ, 1 << 20);  // a pipe: fewer, larger reads (ignored on anything else)
#endif
    std::vector<char>* buf = nullptr;
    size_t fill = 0;
    uint64_t line_in_rec = 0;  // lines of the current record already inside buf[0, scanned)
    size_t scanned = 0, last_cut = 0;
    // FASTQ: blank lines do not count (parse_piece skips them between records, as the mapped and pread routes do);
    // line_start = the byte at `scanned` begins a line
    bool line_start = true;
    auto fresh = [&](size_t at_least) {
      // bound the text in flight (2 x workers pieces); this thread is also the uploader, so full blocks are
      // uploaded while it waits -- the workers may be waiting for exactly that
      std::vector<char>* v = nullptr;
      for (;;) {
        {
          std::unique_lock<std::mutex> g(mu_);
          cv_.wait(g, [&] { return !ready_.empty() || !pool_.empty() || pieces_open_ < 2 * (size_t)nthreads_ + 2 || failed_; });
          if (failed_) break;
          if (ready_.empty()) {
            if (!pool_.empty()) {
              v = pool_.front();
              pool_.pop_front();
            }
            break;
          }
        }
        drain(false);
      }
      if (!v) v = new std::vector<char>(PIECE + std::max<size_t>(PIECE / 8, 1u << 16));
      if (v->size() < at_least + PIECE) v->resize(at_least + PIECE + std::max<size_t>(PIECE / 8, 1u << 16));
      return v;
    };
    buf = fresh(head.size());
    memcpy(buf->data(), head.data(), head.size());
    fill = head.size();
    bool eof = false, need_more = false;
    while (!eof || fill > 0) {
      if (failed_) break;
      // read until the buffer holds a piece (and, after a pass that found no record end, something new)
      while (!eof && (fill < PIECE || need_more)) {
        if (fill == buf->size()) {  // one record longer than the buffer: grow it (a real limit ends the run)
          if (buf->size() >= ((size_t)1 << 31)) die("a FASTQ record is longer than 2 GiB");
          buf->resize(buf->size() * 2);
        }
        const ssize_t n = ::read(fd, buf->data() + fill, buf->size() - fill);
        if (n < 0) {
          if (errno == EINTR) continue;
          die(std::string("read error on input: ") + strerror(errno));
        }
        if (n == 0) eof = true;
        else fill += (size_t)n;
        if (n > 0 && on_stream_bytes) on_stream_bytes(stream_bytes_ += (uint64_t)n);
        need_more = false;
      }
      // last record boundary inside [0, fill): count the new lines (32 bytes per step), then walk to the newline
      // that completes the last whole record
      const char* d = buf->data();
      size_t got = 0, blanks = 0;
      bool st = line_start;
      count_newlines(d + scanned, d + fill, st, got, blanks);
      if (sam_ || blanks == 0) {
        const uint64_t total_lines = line_in_rec + got, recs = total_lines / lines_per_rec;
        if (recs) {
          size_t g2 = 0;
          const char* cut_at = skip_lines_(d + scanned, d + fill, (size_t)(recs * lines_per_rec - line_in_rec), g2);
          last_cut = (size_t)(cut_at - d);
        }
        line_in_rec = total_lines - recs * lines_per_rec;
      } else {  // blank lines: between records they do not count (parse_piece skips them there)
        st = line_start;
        const char* rec_end = nullptr;
        walk_fastq_lines(d + scanned, d + fill, st, line_in_rec, rec_end);
        if (rec_end) last_cut = (size_t)(rec_end - d);
      }
      scanned = fill;
      line_start = st;
      size_t cut = eof ? fill : last_cut;
      if (cut == 0) {
        if (eof) break;
        need_more = true;  // not one whole record yet: keep reading into the same buffer
        continue;
      }
      const size_t rest = fill - cut;
      std::vector<char>* next = fresh(rest);
      memcpy(next->data(), d + cut, rest);
      {
        Piece pc{d, d + cut, buf};
        pc.seq = next_seq_++;
        pc.spool_off = spooled_;
        spooled_ += cut;
        push_piece(pc);
      }
      buf = next;
      fill = rest;
      scanned = rest;  // the carried bytes hold line_in_rec complete lines of an unfinished record (already counted)
      last_cut = 0;
      drain(false);
      if (eof && fill == 0) break;
    }
    {
      std::lock_guard<std::mutex> g(mu_);
      pool_.push_back(buf);
    }
    drain(true);
    return true;
  }
};

// ---- text to the device, parsed there (round 6: SURVEY section 2, kernel K1; rufus_amd/csrc/rfx_text.hip) --------------
// For a regular file of strict 4-line FASTQ counted on one device the host does not parse at all: the mapped text is cut
// into record-aligned pieces (at the cut points only: CountIngest::record_start), the workers copy each piece into
// page-locked memory and queue its host-to-device copy behind the others of the arena that is being filled
// (rfx_text_append: the arena's own stream), and this thread turns every full arena into a read block
// (rfx_text_parse) and hands it to the sink -- while the workers fill the other arena.  What the 16-CPU quota of the
// GPU box spends per read drops from ~1 us of parsing and packing to a memcpy of 330 bytes; the text crosses PCIe at
// ~55 GB/s where the packed blocks of the host route left it idle most of the time.  Text the device refuses (not
// strict 4-line FASTQ after all: a blank line between records, a multi-line record) comes back and goes through the
// caller's host parser, arena by arena: the records of an arena are whole, so nothing is lost or seen twice.
class TextIngest {
  rfx_ctx* ctx_;
  unsigned nthreads_;
  std::function<void(rfx_reads*)> sink_;
  std::function<void(const char*, size_t)> host_text_;
  size_t piece_;
  struct Arena {
    rfx_text* t = nullptr;
    uint64_t gen = 0;  // bumped at every reset: a worker's ticket of an earlier generation is a copy long done
    int state = 0;     // 0 free, 1 filling, 2 full (waiting for this thread)
  };
  Arena arena_[2];
  int filling_ = -1;
  std::deque<int> full_;
  struct Piece {
    const char* b;
    const char* e;
    int fd = -1;  // >= 0: bytes [lo, hi) of a regular file -- the worker reads them itself (pread into its page-locked
    uint64_t lo = 0, hi = 0, fsize = 0;  // buffer) and appends the records that START inside the range
  };
  std::deque<Piece> work_;
  size_t pieces_open_ = 0;
  bool closing_ = false;
  std::atomic<bool> failed_{false};
  std::string fail_msg_;
  std::mutex mu_;
  std::condition_variable cv_;
  std::vector<std::thread> workers_;
  uint64_t reads_ = 0, host_bytes_ = 0;
  static constexpr uint64_t TAIL = 1u << 20;  // longest record a range's tail may hold (feed_file)
  double t_parse_ = 0, t_sink_ = 0;  // this thread: inside rfx_text_parse (it waits for the arena's copies) / in the sink
  unsigned n_arenas_ = 0;
  // the workers, summed (ns): copying a piece into page-locked memory, waiting for the lock + an arena with room, inside
  // rfx_text_append, waiting for the copy that last read the buffer
  std::atomic<uint64_t> w_memcpy_{0}, w_room_{0}, w_append_{0}, w_settle_{0}, w_idle_{0};
  static uint64_t now_ns() { return (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

  void fail(const std::string& m) {
    std::lock_guard<std::mutex> g(mu_);
    if (!failed_.exchange(true)) fail_msg_ = m;
    cv_.notify_all();
  }

  void worker() {
    struct Buf { char* p = nullptr; int arena = -1; uint64_t gen = 0; long ticket = -1; } buf[2];
    const size_t cap = piece_ + TAIL + (1u << 20);
    for (Buf& b : buf) {
      b.p = (char*)rfx_host_alloc(cap);
      if (!b.p) return fail("cannot allocate page-locked text buffers");
    }
    // true: the copy that last read the buffer is done (or belonged to an arena that has been parsed since)
    auto settle = [&](Buf& b) -> bool {
      if (b.ticket < 0) return true;
      auto same_gen = [&] {
        std::lock_guard<std::mutex> g(mu_);
        return arena_[b.arena].gen == b.gen;
      };
      if (same_gen() && rfx_text_wait(arena_[b.arena].t, b.ticket) != RFX_OK && same_gen()) {
        fail(std::string("rfx_text_wait: ") + rfx_last_error());
        return false;
      }
      b.ticket = -1;
      return true;
    };
    int j = 0;
    for (;;) {
      Piece pc;
      {
        const uint64_t t0 = now_ns();
        std::unique_lock<std::mutex> g(mu_);
        cv_.wait(g, [&] { return !work_.empty() || closing_ || failed_; });
        if (failed_ || (work_.empty() && closing_)) break;
        pc = work_.front();
        work_.pop_front();
        w_idle_ += now_ns() - t0;
      }
      Buf& b = buf[j];
      j ^= 1;
      const uint64_t ta = now_ns();
      if (!settle(b)) break;  // (the copy that last read this buffer)
      const uint64_t tb = now_ns();
      size_t n;
      char* src = b.p;  // what is appended: [src, src + n)
      if (pc.fd >= 0) {
        // one byte before the range (is `lo` a line start?) and, behind it, the tail of the record that straddles `hi`
        const uint64_t from = pc.lo ? pc.lo - 1 : 0, to = std::min<uint64_t>(pc.fsize, pc.hi + TAIL);
        const size_t want = (size_t)(to - from);
        if (pread_all(pc.fd, b.p, want, from) != want) { fail(std::string("read error on input: ") + strerror(errno)); break; }
        const char *tb = b.p, *te = b.p + want;
        const char* s0 = pc.lo ? CountIngest::record_start(tb + 1, tb, te) : tb;
        const char* s1 = pc.hi >= pc.fsize ? te : CountIngest::record_start(tb + (pc.hi - from), tb, te);
        if (pc.hi < pc.fsize && s1 == te && to < pc.fsize) { fail("a FASTQ record is longer than 1 MB"); break; }
        if (s0 > s1) s0 = s1;
        src = const_cast<char*>(s0);
        n = (size_t)(s1 - s0);
        if (n && src[n - 1] != '\n' && pc.hi >= pc.fsize) src[n++] = '\n';  // (a file without a final newline)
      } else {
        n = (size_t)(pc.e - pc.b);
        if (n + 1 > cap) { fail("a FASTQ record is longer than a text buffer"); break; }
        memcpy(b.p, pc.b, n);
        if (n && b.p[n - 1] != '\n') b.p[n++] = '\n';  // (the last line of a file without a final newline)
      }
      const uint64_t tc = now_ns();
      w_settle_ += tb - ta;
      w_memcpy_ += tc - tb;
      {
        std::unique_lock<std::mutex> g(mu_);
        for (;;) {
          if (failed_) break;
          if (filling_ >= 0 && rfx_text_room(arena_[filling_].t) >= n) break;
          if (filling_ >= 0) {  // no room: this arena is this thread's ... the main thread's now
            arena_[filling_].state = 2;
            full_.push_back(filling_);
            filling_ = -1;
            cv_.notify_all();
          }
          int f = -1;
          for (int a = 0; a < 2; ++a)
            if (arena_[a].state == 0) { f = a; break; }
          if (f >= 0) {
            arena_[f].state = 1;
            filling_ = f;
            continue;
          }
          cv_.wait(g);
        }
        if (failed_) break;
        const uint64_t td = now_ns();
        w_room_ += td - tc;
        const long tk = n ? rfx_text_append(arena_[filling_].t, src, n) : rfx_text_append(arena_[filling_].t, b.p, 0);
        w_append_ += now_ns() - td;
        if (tk < 0) {
          g.unlock();
          fail(std::string("rfx_text_append: ") + rfx_strerror((int)tk) + " " + rfx_last_error());
          break;
        }
        b.arena = filling_;
        b.gen = arena_[filling_].gen;
        b.ticket = tk;
        --pieces_open_;
        cv_.notify_all();
      }
    }
    // (the buffers outlive their last copies: wait for them)
    for (Buf& b : buf) {
      (void)settle(b);
      rfx_host_free(b.p);
    }
  }

  void finish_arena(int a) {  // this thread only: parse, hand on, give the arena back
    rfx_text* t = arena_[a].t;
    if (rfx_text_bytes(t)) {
      int strict = 1;
      const auto t0 = std::chrono::steady_clock::now();
      rfx_reads* r = rfx_text_parse(t, RFX_PACK_COUNT, 0, &strict);
      const auto t1 = std::chrono::steady_clock::now();
      t_parse_ += std::chrono::duration<double>(t1 - t0).count();
      ++n_arenas_;
      if (r) {
        reads_ += rfx_reads_count(r);
        sink_(r);
        t_sink_ += std::chrono::duration<double>(std::chrono::steady_clock::now() - t1).count();
      } else if (!strict) {
        std::vector<char> text((size_t)rfx_text_bytes(t));
        if (rfx_text_fetch(t, text.data()) != RFX_OK) die(std::string("rufus_amd: rfx_text_fetch: ") + rfx_last_error());
        host_bytes_ += text.size();
        host_text_(text.data(), text.size());
      } else {
        die(std::string("rufus_amd: rfx_text_parse: ") + rfx_last_error());
      }
    }
    {  // (the generation first: a worker that finds its ticket gone looks at it again before it calls that a failure)
      std::lock_guard<std::mutex> g(mu_);
      ++arena_[a].gen;
    }
    rfx_text_reset(t);
    std::lock_guard<std::mutex> g(mu_);
    arena_[a].state = 0;
    cv_.notify_all();
  }

  // the full arenas that wait; all: until every piece is copied, then the partly filled arena too
  void drain(bool all) {
    for (;;) {
      int a = -1;
      {
        std::unique_lock<std::mutex> g(mu_);
        if (all) cv_.wait(g, [&] { return !full_.empty() || pieces_open_ == 0 || failed_; });
        if (failed_) break;
        if (!full_.empty()) {
          a = full_.front();
          full_.pop_front();
        } else if (all && pieces_open_ == 0) {
          if (filling_ < 0) break;
          a = filling_;
          arena_[a].state = 2;
          filling_ = -1;
        } else {
          break;
        }
      }
      finish_arena(a);
    }
    if (failed_) die("rufus_amd jellyfish: " + fail_msg_);
  }

 public:
  TextIngest(rfx_ctx* ctx, unsigned threads, std::function<void(rfx_reads*)> sink,
             std::function<void(const char*, size_t)> host_text, size_t arena_bytes = (size_t)1 << 30, size_t piece = 8u << 20)
      : ctx_(ctx), nthreads_(threads ? threads : 1), sink_(std::move(sink)), host_text_(std::move(host_text)), piece_(piece) {
    for (Arena& a : arena_) {
      a.t = rfx_text_open(ctx_, arena_bytes);
      if (!a.t) die(std::string("rufus_amd: rfx_text_open: ") + rfx_last_error());
    }
    for (unsigned t = 0; t < nthreads_; ++t) workers_.emplace_back([this] { worker(); });
  }
  ~TextIngest() {
    {
      std::lock_guard<std::mutex> g(mu_);
      closing_ = true;
      cv_.notify_all();
    }
    for (auto& t : workers_) t.join();
    for (Arena& a : arena_) rfx_text_close(a.t);
  }
  uint64_t reads() const { return reads_; }
  uint64_t host_parsed_bytes() const { return host_bytes_; }
  std::string timing() const {
    char b[320];
    snprintf(b, sizeof b, "%u arenas: %.3f s waiting for copies + parsing on the device, %.3f s in the sink (count); workers, "
             "summed: memcpy %.3f s, lock + room %.3f s, rfx_text_append %.3f s, waiting for a buffer's copy %.3f s, for a piece %.3f s", n_arenas_,
             t_parse_, t_sink_, w_memcpy_.load() * 1e-9, w_room_.load() * 1e-9, w_append_.load() * 1e-9, w_settle_.load() * 1e-9,
             w_idle_.load() * 1e-9);
    return b;
  }

  // A whole regular file by descriptor: byte ranges that the workers read themselves, straight into their page-locked
  // buffers -- no mapping whose 4 KB pages have to be faulted in one by one and, worse, torn down again by ONE thread
  // (munmap of a 20 GB mapping: 0.3 s of a count that takes 1.5).  false: the file does not start like strict 4-line
  // FASTQ (nothing consumed).
  bool feed_file(int fd, uint64_t size) {
    const std::vector<uint8_t> head = read_head(fd, size, 1u << 16);
    if (!CountIngest::looks_4line((const char*)head.data(), head.size())) return false;
    for (uint64_t lo = 0; lo < size; lo += piece_) {
      Piece pc{nullptr, nullptr};
      pc.fd = fd;
      pc.lo = lo;
      pc.hi = std::min<uint64_t>(size, lo + piece_);
      pc.fsize = size;
      {
        std::lock_guard<std::mutex> g(mu_);
        work_.push_back(pc);
        ++pieces_open_;
        cv_.notify_all();
      }
      drain(false);
    }
    drain(true);
    return true;
  }

  // A whole regular file, mapped.  false: it does not start like strict 4-line FASTQ (nothing consumed).
  bool feed_mapped(const char* data, size_t size) {
    if (!CountIngest::looks_4line(data, std::min<size_t>(size, 1u << 16))) return false;
    const char *b = data, *e = data + size, *at = b;
    while (at < e) {
      const char* want = at + piece_;
      const char* cut = want >= e ? e : CountIngest::record_start(want, b, e);
      if (cut == e && want < e && (size_t)(e - at) > piece_ + (1u << 20)) {
        // no record start within reach: not the format this route is for -- what is left goes to the host parser whole
        drain(true);
        host_bytes_ += (size_t)(e - at);
        host_text_(at, (size_t)(e - at));
        return true;
      }
      {
        std::lock_guard<std::mutex> g(mu_);
        work_.push_back(Piece{at, cut});
        ++pieces_open_;
        cv_.notify_all();
      }
      at = cut;
      drain(false);
    }
    drain(true);
    return true;
  }
};

// ---- what the device-inflate routes below share -------------------------------------------------------------------------
// (weak, here and in front of the classes: the host test harnesses link an executable's source against stand-in libraries
// that lack some of these; a route's constructor then refuses with one line)
#pragma weak rfx_text_open
#pragma weak rfx_text_close
#pragma weak rfx_text_room
#pragma weak rfx_text_bytes
#pragma weak rfx_text_append
#pragma weak rfx_text_wait
#pragma weak rfx_text_reset
#pragma weak rfx_text_parse
#pragma weak rfx_text_append_bgzf
#pragma weak rfx_text_settle
#pragma weak rfx_text_settle_fasta
#pragma weak rfx_text_parse_fasta

[[noreturn]] inline void die_not_strict() { die("compressed input must be strict 4-line FASTQ: inflate it and pipe it in"); }
[[noreturn]] inline void die_rc(const char* what, int rc) {
  die(std::string("rufus_amd: ") + what + ": " + rfx_strerror(rc) + " " + rfx_last_error());
}

// The knobs both executables read.  RFX_INGEST_PIECE: the compressed (or text) bytes a route hands over at a time, at
// least 1024; unset: the route's default.
inline size_t env_piece(size_t dflt) {
  const char* ev = getenv("RFX_INGEST_PIECE");
  return ev ? (size_t)std::max(1024ll, atoll(ev)) : dflt;
}
// RFX_*_ARENA: the bytes of an arena, clamped to [lo, hi]; unset (or no name): 1 GiB.  Test knobs -- small files cross
// arenas -- and, for RFX_FASTA_ARENA, the way out for genomes whose chromosomes pass the default.  (hi = ARENA_MAX where
// the route's offsets are 32 bits wide.)
static constexpr long long ARENA_MAX = 0xFFFFDFFFll;
inline size_t env_arena(const char* name, long long lo = 1ll << 20, long long hi = std::numeric_limits<long long>::max()) {
  const char* ev = name ? getenv(name) : nullptr;
  return ev ? (size_t)std::min(hi, std::max(lo, atoll(ev))) : (size_t)1 << 30;
}

// The ring of page-locked buffers that compressed bytes go through on their way to an arena: a buffer is copied from
// asynchronously (rfx_text_append_bgzf queues the copy and the inflate), so each remembers the arena and the ticket of
// the copy that last read it, and is handed out again only when that copy is done.  An arena's tickets die with its
// reset: settle_arena comes first.  cap = max(piece, 64 KiB): a BGZF block is at most 64 KiB.
class PinnedRing {
 public:
  struct Buf { char* p = nullptr; rfx_text* t = nullptr; long ticket = -1; };
  PinnedRing(size_t n, size_t piece) : cap_(std::max<size_t>(piece, 1u << 16)), ring_(n) {
    for (Buf& b : ring_) {
      b.p = (char*)rfx_host_alloc(cap_);
      if (!b.p) die("rufus_amd: cannot allocate page-locked buffers for the compressed input");
    }
  }
  PinnedRing(const PinnedRing&) = delete;
  PinnedRing& operator=(const PinnedRing&) = delete;
  ~PinnedRing() {
    settle_all();
    for (Buf& b : ring_) rfx_host_free(b.p);
  }
  size_t cap() const { return cap_; }
  Buf& take() {  // the next buffer, round robin, settled
    Buf& b = ring_[next_];
    next_ = (next_ + 1) % ring_.size();
    settle(b);
    return b;
  }
  static void sent(Buf& b, rfx_text* arena, long ticket) {
    b.t = arena;
    b.ticket = ticket;
  }
  void settle_arena(rfx_text* t) {  // before an arena is reset
    for (Buf& b : ring_)
      if (b.t == t) settle(b);
  }
  void settle_all() {  // before the arenas are closed
    for (Buf& b : ring_) settle(b);
  }

 private:
  static void settle(Buf& b) {
    if (b.ticket >= 0 && rfx_text_wait(b.t, b.ticket) != RFX_OK) die(std::string("rufus_amd: rfx_text_wait: ") + rfx_last_error());
    b.ticket = -1;
  }
  size_t cap_, next_ = 0;
  std::vector<Buf> ring_;
};

// The run rule.  One cheap pass over the block headers (rfx_bgzf_scan) cuts [from, to) of a mapped BGZF file into runs of
// whole blocks, in file order: at most max_bytes compressed bytes (a ring buffer) and at most max_blocks blocks each --
// bgzf_run_blocks(arena): a quarter of an arena of inflated bytes, and at least one block.  *blocks and *inflated (either
// may be null) grow by what the runs hold.  Dies, with the caller's prefix, on a block that is not BGZF or not whole.
struct BgzfRun { size_t at, n; uint64_t inflated; };
inline uint32_t bgzf_run_blocks(uint64_t arena_bytes) { return (uint32_t)std::max<uint64_t>(1, arena_bytes / 4 / 65536); }
inline std::vector<BgzfRun> bgzf_runs(const char* m, size_t from, size_t to, size_t max_bytes, uint32_t max_blocks, const std::string& who,
                                      uint64_t* blocks, uint64_t* inflated = nullptr) {
  std::vector<BgzfRun> runs;
  for (size_t at = from; at < to;) {
    uint32_t nb = 0;
    uint64_t used = 0, inf = 0;
    const int rc = rfx_bgzf_scan(m + at, std::min(to - at, max_bytes), max_blocks, &nb, &used, &inf);
    if (nb == 0) die(who + (rc == RFX_OK ? "truncated" : "no") + " BGZF block at byte " + std::to_string(at) + " of the compressed input");
    runs.push_back({at, (size_t)used, inf});
    if (blocks) *blocks += nb;
    if (inflated) *inflated += inf;
    at += (size_t)used;
  }
  return runs;
}
// The fill.  Queues runs[i], runs[i + 1], ... into arena `a` until the next does not fit: a settled buffer of the ring,
// memcpy, rfx_text_append_bgzf -- queued, nothing waited for.  true: runs[i] is left (the arena is full, or smaller than
// the run); false: the file is at its end.  An append the library refuses goes to `refuse`.
inline bool bgzf_fill(PinnedRing& ring, rfx_text* a, const char* m, const std::vector<BgzfRun>& runs, size_t& i, uint64_t& appends,
                      void (*refuse)(const char*, int) = die_rc) {
  for (; i < runs.size(); ++i) {
    const BgzfRun& r = runs[i];
    if (r.inflated > rfx_text_room(a)) return true;
    PinnedRing::Buf& b = ring.take();
    memcpy(b.p, m + r.at, r.n);
    const long tk = rfx_text_append_bgzf(a, b.p, r.n);
    if (tk < 0) refuse("rfx_text_append_bgzf", (int)tk);
    PinnedRing::sent(b, a, tk);
    ++appends;
  }
  return false;
}

// A page-locked buffer that grows: what a gather writes into.  The gathers answer RFX_E_RANGE with the size they need;
// need() then makes room for that and a quarter more, and the caller asks again.
struct PinnedBuf {
  void* p = nullptr;
  size_t cap = 0;
  PinnedBuf() = default;
  PinnedBuf(const PinnedBuf&) = delete;
  PinnedBuf& operator=(const PinnedBuf&) = delete;
  void need(size_t bytes) {
    if (bytes <= cap) return;
    if (p) rfx_host_free(p);
    cap = bytes + bytes / 4 + 4096;
    p = rfx_host_alloc(cap);
    if (!p) die("rufus_amd: cannot allocate page-locked memory for the pulled records");
  }
  ~PinnedBuf() { if (p) rfx_host_free(p); }
};

// The two text arenas of a route that counts compressed FASTQ (or, fasta: FASTA) text, and what happens to a full one.
// Blocks and chunks end anywhere: a full arena is cut at its last whole record (rfx_text_settle; FASTA: at its last header
// line, rfx_text_settle_fasta, so the last record always moves on), the tail moves to the front of the other arena, and
// the arena is parsed, handed to the sink and reset -- behind the tickets of `ring`, where the route has one.  Two arenas:
// one thread feeds, settles, parses and sinks, so a third would never be filled while two are busy.  What a route does
// between cut() and parse_and_sink() -- filling the other arena -- is the route's.
// Strict 4-line FASTQ only: the carry rule counts four lines per record, and text the device parser refuses cannot be
// handed to the host parser arena by arena (an arena's cut would be wrong to begin with).  FASTA: every step parses at
// least one record or ends the run: a record that does not fit an arena is refused, not cut.
class TextArenaPair {
  rfx_text* arena_[2] = {nullptr, nullptr};
  std::function<void(rfx_reads*)> sink_;
  uint64_t bytes_;
  bool fasta_;
  PinnedRing* ring_;
  uint64_t arenas_ = 0, reads_ = 0;

 public:
  TextArenaPair(std::function<void(rfx_reads*)> sink, uint64_t arena_bytes, bool fasta = false, PinnedRing* ring = nullptr)
      : sink_(std::move(sink)), bytes_(arena_bytes), fasta_(fasta), ring_(ring) {}
  void open(rfx_ctx* ctx) {  // (not the constructor's: a route refuses a library that cannot serve it first)
    for (rfx_text*& a : arena_) {
      a = rfx_text_open(ctx, bytes_);
      if (!a) die(std::string("rufus_amd: rfx_text_open: ") + rfx_last_error());
    }
  }
  ~TextArenaPair() {
    if (ring_) ring_->settle_all();
    for (rfx_text* a : arena_)
      if (a) rfx_text_close(a);
  }
  rfx_text* operator[](int i) const { return arena_[i]; }
  uint64_t bytes() const { return bytes_; }
  uint64_t arenas() const { return arenas_; }
  uint64_t reads() const { return reads_; }

  [[noreturn]] void too_long() const {
    char msg[160];
    snprintf(msg, sizeof msg, "rufus_amd jellyfish count: a FASTA sequence does not fit a text arena of %llu bytes (RFX_FASTA_ARENA)",
             (unsigned long long)bytes_);
    die(msg);
  }
  [[noreturn]] void no_record() const { fasta_ ? too_long() : die_not_strict(); }  // text that no arena holds a whole record of

  // cuts t behind its last whole record; the bytes moved to `next` (null: the input ends here, nothing may be left)
  uint64_t settle(rfx_text* t, rfx_text* next) {
    uint64_t carried = 0;
    const int rc = fasta_ ? rfx_text_settle_fasta(t, next, &carried) : rfx_text_settle(t, next, &carried);
    // (a block that did not inflate: only an arena that BGZF blocks went into says so)
    if (rc == RFX_E_FORMAT && !strncmp(rfx_last_error(), "rfx_bgzf:", 9)) die(std::string("rufus_amd jellyfish count: ") + rfx_last_error());
    if (fasta_ && rc == RFX_E_RANGE) too_long();  // (one record fills the arena, or its tail does not fit the next)
    if (fasta_ && rc != RFX_OK)
      die(std::string("rufus_amd jellyfish count: rfx_text_settle_fasta: ") + rfx_strerror(rc) + " " + rfx_last_error());
    if (rc == RFX_E_FORMAT || rc == RFX_E_RANGE) die_not_strict();  // (ends inside a record / a "record" longer than an arena)
    if (rc != RFX_OK) die_rc("rfx_text_settle", rc);
    return carried;
  }
  void cut(rfx_text* t, rfx_text* next) {  // a full arena
    const uint64_t before = rfx_text_bytes(t);
    if (settle(t, next) == before) no_record();  // a full arena without one whole record
  }
  void parse_and_sink(rfx_text* t) {
    if (rfx_text_bytes(t)) {
      int strict = 1;
      rfx_reads* r = fasta_ ? rfx_text_parse_fasta(t, RFX_PACK_COUNT, &strict) : rfx_text_parse(t, RFX_PACK_COUNT, 0, &strict);
      if (!r && !strict && fasta_) die("rufus_amd jellyfish count: the inflated text does not begin with '>'");
      if (!r && !strict) die_not_strict();
      if (!r) die(std::string(fasta_ ? "rufus_amd: rfx_text_parse_fasta: " : "rufus_amd: rfx_text_parse: ") + rfx_last_error());
      reads_ += rfx_reads_count(r);
      ++arenas_;
      sink_(r);
    }
    if (ring_) ring_->settle_arena(t);
    rfx_text_reset(t);
  }
  // The end of the input, in arena `cur`.  FASTQ: a file without a final newline gets one -- what is left behind the last
  // whole record moves to the other arena, the newline goes behind it, and that arena is the last.  FASTA: nothing is
  // carried, and a last line without '\n' is a line.
  void finish(int cur) {
    rfx_text* t = arena_[cur];
    rfx_text* nx = arena_[cur ^ 1];
    if (fasta_) {
      (void)settle(t, nullptr);
      parse_and_sink(t);
      return;
    }
    if (settle(t, nx)) {
      const long tk = rfx_text_append(nx, "\n", 1);
      if (tk < 0 || rfx_text_wait(nx, tk) != RFX_OK) die(std::string("rufus_amd: rfx_text_append: ") + rfx_last_error());
      parse_and_sink(t);
      (void)settle(nx, nullptr);
      parse_and_sink(nx);
    } else {
      parse_and_sink(t);
    }
  }
};

// ---- bgzip'd FASTQ: inflated on the device (rfx_text_append_bgzf; rufus_amd/csrc/rfx_bgzf.hip) -------------------------
// Replaces `zcat F.fastq.gz | jellyfish count ... /dev/stdin` (runRufus.sh:157-160): the host only reads the file.  The
// run rule (bgzf_runs) cuts the mapped file; the runs go, IN FILE ORDER (records straddle blocks, so the text must arrive
// in order), through a PinnedRing into the arena of a TextArenaPair that is being filled (bgzf_fill).  A full arena is
// cut, then the next one is filled -- its copies and inflate kernels queued, nothing waited for -- BEFORE the cut arena is
// parsed and counted, so the device inflates the next arena's text beside the count of this one.
// (without rfx_text_append_bgzf and rfx_text_settle -- a stand-in library that has the text arena but no device -- BGZF
// input is refused by the constructor)
//
// bgzip'd FASTA (fasta = true; rufus_amd/csrc/rfx_fasta.hip): the same runs, ring and steps, the pair in its FASTA mode.
// Replaces `zcat ref.fa.gz | jellyfish count ... /dev/stdin` in front of the -e / -f databases (runRufus.sh:77, :115).
// (without rfx_text_settle_fasta and rfx_text_parse_fasta the FASTA route refuses with one line)
class BgzfIngest {
  bool fasta_;
  PinnedRing ring_;  // (in front of the pair: the pair settles it before the arenas close)
  TextArenaPair pair_;
  uint64_t blocks_ = 0, appends_ = 0;

 public:
  BgzfIngest(rfx_ctx* ctx, std::function<void(rfx_reads*)> sink, size_t arena_bytes = (size_t)1 << 30, size_t piece = 8u << 20,
             bool fasta = false)
      : fasta_(fasta), ring_(4, piece), pair_(std::move(sink), arena_bytes, fasta, &ring_) {
    if (!rfx_text_append_bgzf || !rfx_text_settle) die("rufus_amd jellyfish count: this library cannot inflate BGZF input");
    if (fasta_ && (!rfx_text_settle_fasta || !rfx_text_parse_fasta)) die("rufus_amd jellyfish count: this library cannot read bgzip'd FASTA");
    pair_.open(ctx);
  }
  uint64_t reads() const { return pair_.reads(); }
  std::string counts() const {
    char b[160];
    snprintf(b, sizeof b, fasta_ ? "fasta route: %llu blocks in %llu appends, %llu arenas, %llu sequences"
                                 : "bgzf route: %llu blocks in %llu appends, %llu arenas, %llu reads",
             (unsigned long long)blocks_, (unsigned long long)appends_, (unsigned long long)pair_.arenas(), (unsigned long long)pair_.reads());
    return b;
  }

  // A whole mapped BGZF file.  Dies on a block that is not BGZF or not whole, on text that is not strict 4-line FASTQ
  // and on a block that does not inflate.
  void feed_mapped(const char* m, size_t size) {
    const std::vector<BgzfRun> runs =
        bgzf_runs(m, 0, size, ring_.cap(), bgzf_run_blocks(pair_.bytes()), "rufus_amd jellyfish count: ", &blocks_);
    int cur = 0;
    size_t i = 0;
    auto fill = [&](rfx_text* a) {
      const bool more = bgzf_fill(ring_, a, m, runs, i, appends_);
      // A run that no arena holds.  A run is a quarter of an arena of text at most, but one block at least: below 256 KiB
      // a run may pass the quarter, and below the 64 KiB that one block may inflate to, the arena.
      if (more && runs[i].inflated > pair_.bytes()) pair_.no_record();
      return more;
    };
    bool more = fill(pair_[cur]);
    while (more) {
      pair_.cut(pair_[cur], pair_[cur ^ 1]);
      more = fill(pair_[cur ^ 1]);  // queued, not waited for: the device inflates it beside this arena's count
      pair_.parse_and_sink(pair_[cur]);
      cur ^= 1;
    }
    pair_.finish(cur);
  }
};

// The first inflated byte of a BGZF file, or -1: what sends a bgzip'd input of `jellyfish count` to the FASTA route ('>')
// or where it went before (anything else), as is_bam does for BAM.  The first non-empty block is inflated by the host side
// of rfx_bgzf_core.h (a serial copy as its output policy); -1 when no such block lies whole in the file's first 128 KiB or
// it does not inflate -- the route that takes the file then says what is wrong with it.
inline int bgzf_first_byte(int fd, uint64_t size) {
  const std::vector<uint8_t> head = read_head(fd, size, 1u << 17);
  const size_t got = head.size();
  struct Serial {
    uint8_t* out;
    void literal(uint32_t pos, uint32_t byte) { out[pos] = (uint8_t)byte; }
    void match(uint32_t pos, uint32_t len, uint32_t dist) {
      for (uint32_t i = 0; i < len; ++i) out[pos + i] = out[pos - dist + i % dist];
    }
    void stored(uint32_t pos, const uint8_t* src, uint32_t n) { memcpy(out + pos, src, n); }
    void end() {}
  };
  for (size_t at = 0; at < got;) {
    uint32_t bsize = 0, pay_off = 0, pay_len = 0, isize = 0, crc = 0;
    if (bgzf_block_header(head.data() + at, got - at, &bsize, &pay_off, &pay_len, &isize, &crc) != 0) return -1;
    if (isize) {
      std::vector<uint8_t> out(isize);
      std::unique_ptr<bgzf_tables> tables(new bgzf_tables());
      Serial so{out.data()};
      const uint8_t* p = head.data() + at + pay_off;
      if (bgzf_inflate(p, p + pay_len, isize, *tables, so) != BGZF_OK) return -1;
      return out[0];
    }
    at += bsize;
  }
  return -1;
}

// ---- plain-gzip FASTQ: inflated on the device (rfx_text_append_gzip; rufus_amd/csrc/rfx_gzip.hip) -------------------------
// Replaces `zcat F.fastq.gz | jellyfish count ... /dev/stdin` (runRufus.sh:157-160, :229-232) for files that are gzip but
// not BGZF: what a sequencer or an archive hands out.  BgzfIngest's TextArenaPair, without a ring; what differs is the
// fill: the stream has no block index, so the mapped file is PRESENTED, a piece
// at a time, and rfx_text_append_gzip says how many of the piece's bytes are done with -- it appends whole confirmed chunks
// only.  Nothing consumed and nothing appended is either a full arena (rfx_gzip_need() != 0: settle and switch) or a piece
// that holds no whole chunk (a stream of stored or fixed blocks has no chunk starts to find: the piece doubles, up to the
// rest of the file).  The append waits for the device, so the inflate of the next arena does not overlap this arena's
// count.  (weak: as BgzfIngest's)
#pragma weak rfx_gzip_open
#pragma weak rfx_gzip_close
#pragma weak rfx_text_append_gzip
#pragma weak rfx_gzip_need
#pragma weak rfx_gzip_stats
class GzipIngest {
  rfx_ctx* ctx_;
  size_t piece_;
  TextArenaPair pair_;
  uint64_t appends_ = 0, files_ = 0;
  uint64_t stats_[8] = {0, 0, 0, 0, 0, 0, 0, 0};

 public:
  GzipIngest(rfx_ctx* ctx, std::function<void(rfx_reads*)> sink, size_t arena_bytes = (size_t)1 << 30, size_t piece = 128u << 20)
      : ctx_(ctx), piece_(std::max<size_t>(piece, 64)), pair_(std::move(sink), arena_bytes) {
    if (!rfx_gzip_open || !rfx_gzip_close || !rfx_text_append_gzip || !rfx_gzip_need || !rfx_gzip_stats || !rfx_text_settle)
      die("rufus_amd jellyfish count: this library cannot inflate plain-gzip input");
    pair_.open(ctx_);
  }
  uint64_t reads() const { return pair_.reads(); }
  std::string counts() const {
    char b[320];
    snprintf(b, sizeof b,
             "gzip route: %llu files, %llu appends, %llu arenas, %llu reads; chunks found %llu, confirmed %llu, dropped %llu, "
             "inserted %llu, rounds %llu, members %llu, batches %llu, bytes %llu",
             (unsigned long long)files_, (unsigned long long)appends_, (unsigned long long)pair_.arenas(), (unsigned long long)pair_.reads(),
             (unsigned long long)stats_[0], (unsigned long long)stats_[1], (unsigned long long)stats_[2], (unsigned long long)stats_[3],
             (unsigned long long)stats_[4], (unsigned long long)stats_[5], (unsigned long long)stats_[6], (unsigned long long)stats_[7]);
    return b;
  }

  // A whole mapped plain-gzip file.  Dies on what rfx_text_append_gzip refuses (its "rfx_gzip:" text) and on text that is
  // not strict 4-line FASTQ.
  void feed_mapped(const char* m, size_t size) {
    rfx_gzip* gz = rfx_gzip_open(ctx_);
    if (!gz) die(std::string("rufus_amd: rfx_gzip_open: ") + rfx_last_error());
    ++files_;
    int cur = 0;
    size_t at = 0, piece = piece_;
    uint64_t fresh = 0;  // bytes this file has put into the current arena
    double ratio = 4.0;  // inflated / compressed bytes, the largest seen
    auto next_arena = [&] {  // the arena's tail moves on, it is counted, the other one is filled
      pair_.cut(pair_[cur], pair_[cur ^ 1]);
      pair_.parse_and_sink(pair_[cur]);
      cur ^= 1;
      fresh = 0;
    };
    while (at < size) {
      const size_t n = std::min(piece, size - at);
      // a piece that will not fit what is left of the arena would be found and walked twice: the arena goes as it is
      if (fresh && (double)n * ratio > (double)rfx_text_room(pair_[cur])) next_arena();
      rfx_text* a = pair_[cur];
      uint64_t used = 0;
      const long got = rfx_text_append_gzip(a, gz, m + at, n, at + n == size, &used);
      ++appends_;
      if (got == RFX_E_FORMAT && !strncmp(rfx_last_error(), "rfx_gzip:", 9)) die(std::string("rufus_amd jellyfish count: ") + rfx_last_error());
      if (got < 0) die(std::string("rufus_amd: rfx_text_append_gzip: ") + rfx_strerror((int)got) + " " + rfx_last_error());
      at += (size_t)used;
      fresh += (uint64_t)got;
      if (used >= 65536) ratio = std::max(ratio, 1.05 * (double)got / (double)used);
      if (got || used) continue;
      if (rfx_gzip_need(gz)) {  // the arena is full
        next_arena();
      } else if (n == size - at) {
        die("rufus_amd jellyfish count: rfx_text_append_gzip made no progress at the end of the file");  // (it reports such a file itself)
      } else {
        piece *= 2;  // no whole chunk in the piece
      }
    }
    uint64_t st[8];
    if (rfx_gzip_stats(gz, st) == RFX_OK)
      for (int i = 0; i < 8; ++i) stats_[i] += st[i];
    rfx_gzip_close(gz);
    pair_.finish(cur);
  }
};

// The first inflated byte of a plain-gzip file, or -1: what lets `jellyfish count` refuse anything but FASTQ ('@') before
// the device sees it.  The first member's header, then the host side of rfx_gzip_core.h over the file's first 64 KiB with
// an output policy that keeps byte 0.
inline int gzip_first_byte(int fd, uint64_t size) {
  const std::vector<uint8_t> head = read_head(fd, size, 1u << 16);
  const size_t got = head.size();
  struct First {
    int byte = -1;
    void literal(uint64_t pos, uint32_t b) { if (pos == 0) byte = (int)b; }
    void match(uint64_t, uint32_t, uint32_t) {}
    void stored(uint64_t pos, const uint8_t* src, uint32_t) { if (pos == 0) byte = src[0]; }
    void end() {}
  };
  uint64_t hl = 0;
  if (gz_member_header(head.data(), got, &hl) != 0) return -1;
  std::unique_ptr<bgzf_tables> tables(new bgzf_tables());
  First f;
  gz_result r;
  gz_run(head.data(), head.data() + got, hl * 8u, hl * 8u + 1u, true, ~0ull, *tables, f, r);  // (the first block, or what of it is there)
  return f.byte;
}

// ---- BAM: inflated, its records found and their sequences packed on the device (rfx_bam_*; rufus_amd/csrc/rfx_bam.hip) --
// Replaces `samtools view -F 3328 X.bam | PassThroughSamCheck CHR | jellyfish count ... /dev/fd/0` (runRufus.sh:599,
// scripts/RunJellyForRUFUS.sh:28-29): the host only reads the file.  BgzfIngest's shape -- the run rule, the ring of
// page-locked buffers, two arenas, settle -> fill the next arena -> parse and sink -- with rfx_bam_settle for the carry
// (a record straddles blocks and arenas as a FASTQ record does) and rfx_bam_parse for the block.  The runs start at the
// block rfx_bam_header names; `skip`, the header's bytes in that block, goes to the first arena's settle only.  The
// chromosome log of PassThroughSamCheck (src/PassThroughSamCheck.cpp:140-155) is stitched on the host from the arenas'
// run lists: a run that begins an arena with the refID the arena before ended with is no change.
//
// set_region (`samtools view -F N X.bam REGION` in front of the feeder, runRufus.sh -R): the header is read as ever; the
// runs of blocks then begin at the block of the index's START (rfx_bai.hpp: one range per region) with `skip` = START's
// offset inside it, and end with STOP's block.  Every settled arena gets rfx_bam_set_region before anything looks at its
// records, so the index decides what is inflated and nothing else.  Without a usable index the whole file is walked.
// The last arena of a range may end inside a record -- STOP's block holds whatever follows the region -- which is accepted
// only where that record starts at or behind STOP.
// (weak, as above: the host harnesses link the executable's source against stand-in libraries without these)
#pragma weak rfx_bam_header
#pragma weak rfx_bam_settle
#pragma weak rfx_bam_parse
#pragma weak rfx_bam_set_region
#pragma weak rfx_bam_parse_filter
#pragma weak rfx_bam_name_hashes
#pragma weak rfx_bam_locate
#pragma weak rfx_reads_get
#pragma weak rfx_reads_words
class BamIngest {
  rfx_ctx* ctx_;
  std::function<void(rfx_reads*)> sink_;
  uint32_t exclude_;
  rfx_text* arena_[2] = {nullptr, nullptr};
  uint64_t arena_bytes_;
  PinnedRing ring_;
  uint64_t blocks_ = 0, arenas_ = 0, records_ = 0, reads_ = 0, appends_ = 0;
  int32_t n_ref_ = 0;
  std::vector<std::string> ref_names_;
  std::vector<int32_t> chr_runs_;  // the kept records' refID wherever it changes, over the whole input
  std::vector<uint32_t> runs_buf_;
  // `RUFUS.Filter --bam` (BamPairFilter below) walks the same arenas with another step per arena: when set, it is called
  // for every settled arena instead of rfx_bam_parse + sink, and reports the arena's kept records
  std::function<uint64_t(rfx_text*, uint64_t)> per_arena_;
  std::string tool_ = "rufus_amd jellyfish count";
  // set_keep_packed (`jellyfish count --bam CHR --keep-packed FILE`; rfx_bam_cache.hpp): every settled arena with kept
  // records also leaves a chunk of FILE -- the filter's view of the records (rfx_bam_parse_filter for MinQ), their name
  // hashes and their addresses -- so that `RUFUS.Filter --packed FILE` need not inflate the file twice more
  // (runRufus.sh:964-967 after scripts/RunJellyForRUFUS.sh:28-29)
  int cache_fd_ = -1, cache_minq_ = 0;
  rfxbamcache::Writer cache_;
  // set_region
  bool region_on_ = false, region_quiet_ = false;
  std::string region_text_, bam_path_;
  const char* region_index_ = "none";  // none | used | unusable
  rfxbai::Region region_;
  uint64_t in_region_ = 0;
  struct KeepBufs {
    std::vector<uint64_t> hash, codes;
    std::vector<uint32_t> start, bytes, len, word_off, good, runs;
  } keep_;

  [[noreturn]] void cache_write_error() { die(tool_ + ": write error on the packed-read cache: " + strerror(errno)); }
  // base: the stream offset of the arena's byte 0
  void keep_chunk(rfx_text* t, uint64_t n_records, uint64_t base) {
    keep_.runs.resize((size_t)2 * n_records);
    uint64_t n_runs = 0;
    rfx_reads* rd = rfx_bam_parse_filter(t, exclude_, cache_minq_, keep_.runs.data(), n_records, &n_runs);
    if (!rd) die(tool_ + ": --keep-packed: " + rfx_last_error());
    const uint32_t n = rfx_reads_count(rd);
    const uint64_t words = rfx_reads_words(rd);
    if (n == 0) {  // (an arena none of whose records is kept leaves no chunk)
      rfx_reads_free(rd);
      return;
    }
    keep_.codes.resize((size_t)words + 1);
    keep_.good.resize((size_t)words + 1);
    keep_.word_off.resize((size_t)n + 1);
    keep_.len.resize(n);
    keep_.hash.resize(n);
    keep_.start.resize(n);
    keep_.bytes.resize(n);
    int rc = rfx_reads_get(rd, keep_.codes.data(), nullptr, keep_.good.data(), keep_.word_off.data(), keep_.len.data());
    rfx_reads_free(rd);
    if (rc != RFX_OK) die(tool_ + ": --keep-packed: rfx_reads_get: " + rfx_last_error());
    uint64_t got = 0;
    rc = rfx_bam_name_hashes(t, exclude_, nullptr, n, keep_.hash.data(), n, &got);
    if (rc != RFX_OK || got != n) die(tool_ + ": --keep-packed: rfx_bam_name_hashes: " + rfx_last_error());
    rc = rfx_bam_locate(t, exclude_, n, keep_.start.data(), keep_.bytes.data());
    if (rc != RFX_OK) die(tool_ + ": --keep-packed: rfx_bam_locate: " + rfx_last_error());
    rfxbamcache::Chunk c;
    c.stream_off = base;
    c.n = n;
    c.n_words = (uint32_t)words;
    c.n_runs = (uint32_t)n_runs;
    c.hash = keep_.hash.data();
    c.start = keep_.start.data();
    c.rbytes = keep_.bytes.data();
    c.len = keep_.len.data();
    c.word_off = keep_.word_off.data();
    c.codes = keep_.codes.data();
    c.good = keep_.good.data();
    c.runs = keep_.runs.data();
    if (!cache_.add_chunk(c)) cache_write_error();
  }

  void parse_and_sink(rfx_text* t, uint64_t n_records, uint64_t base) {
    if (n_records && cache_fd_ >= 0) keep_chunk(t, n_records, base);
    if (n_records && per_arena_) {
      reads_ += per_arena_(t, n_records);
      records_ += n_records;
      ++arenas_;
    } else if (n_records) {
      runs_buf_.resize((size_t)2 * n_records);
      uint64_t n_runs = 0;
      rfx_reads* r = rfx_bam_parse(t, exclude_, runs_buf_.data(), n_records, &n_runs);
      if (!r) die(tool_ + ": " + rfx_last_error());
      add_runs(runs_buf_.data(), n_runs);
      reads_ += rfx_reads_count(r);
      records_ += n_records;
      ++arenas_;
      sink_(r);
    }
    ring_.settle_arena(t);
    rfx_text_reset(t);
  }
  // the whole records of t; *carried = the bytes moved to `next`
  uint64_t settle(rfx_text* t, rfx_text* next, uint64_t skip, uint64_t* carried) {
    uint64_t n_records = 0;
    const int rc = rfx_bam_settle(t, next, skip, n_ref_, &n_records, carried);
    if (rc == RFX_E_FORMAT) die(tool_ + ": --bam: " + rfx_last_error());
    if (rc == RFX_E_RANGE) die(tool_ + ": --bam: a record that is longer than an arena");
    if (rc != RFX_OK) die(std::string("rufus_amd: rfx_bam_settle: ") + rfx_strerror(rc) + " " + rfx_last_error());
    if (region_on_) {
      uint64_t n_in = 0;
      const int rr = rfx_bam_set_region(t, region_.tid, region_.beg, region_.end, &n_in);
      if (rr != RFX_OK) die(std::string("rufus_amd: rfx_bam_set_region: ") + rfx_strerror(rr) + " " + rfx_last_error());
      in_region_ += n_in;
    }
    return n_records;
  }

  // one whole BGZF block at compressed byte `at` of the file: its compressed and inflated sizes
  static bool block_at(const char* m, size_t size, uint64_t at, uint64_t* used, uint64_t* inflated) {
    if (at >= size) return false;
    uint32_t nb = 0;
    *used = *inflated = 0;
    (void)rfx_bgzf_scan(m + at, std::min<size_t>(size - (size_t)at, 1u << 16), 1, &nb, used, inflated);
    return nb == 1;
  }
  // The file range of the region: X.bam.bai, then X.bai.  false: no usable index (one line on stderr), the whole file is
  // walked.  true: *empty, or the blocks [*start_c, *end_c) with *skip in the first; *stop_in = STOP's offset inside the
  // last block's inflated data (0: STOP is that block's end), *stop_inf the last block's inflated size.
  bool region_range(const char* m, size_t size, uint64_t first_block, uint32_t skip0, bool* empty, uint64_t* start_c, uint64_t* skip,
                    uint64_t* end_c, uint64_t* stop_in, uint64_t* stop_inf) {
    std::vector<std::string> tries{bam_path_ + ".bai"};
    if (bam_path_.size() > 4 && bam_path_.compare(bam_path_.size() - 4, 4, ".bam") == 0)
      tries.push_back(bam_path_.substr(0, bam_path_.size() - 4) + ".bai");
    std::vector<uint8_t> bytes;
    std::string found;
    for (const std::string& path : tries) {
      FILE* f = fopen(path.c_str(), "rb");
      if (!f) continue;
      uint8_t buf[1 << 16];
      for (size_t n; (n = fread(buf, 1, sizeof buf, f)) > 0;) bytes.insert(bytes.end(), buf, buf + n);
      fclose(f);
      found = path;
      break;
    }
    if (found.empty()) {
      if (!region_quiet_) fprintf(stderr, "%s: --region: '%s' has no .bai index: walking the whole file\n", tool_.c_str(), bam_path_.c_str());
      return false;
    }
    auto unusable = [&](const std::string& why) {
      region_index_ = "unusable";
      if (!region_quiet_)
        fprintf(stderr, "%s: --region: '%s' is not a usable BAM index (%s): walking the whole file\n", tool_.c_str(), found.c_str(),
                why.c_str());
      return false;
    };
    rfxbai::Index ix;
    std::string why;
    if (!rfxbai::read_index(bytes.data(), bytes.size(), n_ref_, size, &ix, &why)) return unusable(why);
    const rfxbai::Range r = rfxbai::query(ix, region_.tid, region_.beg, region_.end);
    *empty = r.empty;
    if (!r.empty) {
      // the two ends name blocks of THIS file, behind its header
      uint64_t used = 0, inf = 0;
      *start_c = r.start >> 16;
      *skip = r.start & 0xFFFFu;
      if (r.start < ((first_block << 16) | skip0)) return unusable("a chunk in front of the first record");
      if (!block_at(m, size, *start_c, &used, &inf) || *skip > inf) return unusable("a chunk that starts at no BGZF block");
      *stop_in = r.stop & 0xFFFFu;
      *stop_inf = 0;
      *end_c = r.stop >> 16;
      if (*stop_in) {
        if (!block_at(m, size, *end_c, &used, &inf) || *stop_in > inf) return unusable("a chunk that ends at no BGZF block");
        *end_c += used;
        *stop_inf = inf;
      }
    }
    region_index_ = "used";
    return true;
  }

 public:
  // before feed_mapped: only the records that overlap `text` (rfx_bai.hpp parse_region) are kept; bam_path: the file
  // feed_mapped is given, whose index is looked for beside it.  quiet: the stderr line about the index is not repeated.
  void set_region(const std::string& text, const std::string& bam_path, bool quiet = false) {
    if (!rfx_bam_set_region) die(tool_ + ": this library cannot restrict BAM input to a region");
    region_on_ = true;
    region_quiet_ = quiet;
    region_text_ = text;
    bam_path_ = bam_path;
  }
  BamIngest(rfx_ctx* ctx, std::function<void(rfx_reads*)> sink, uint32_t exclude_flags, size_t arena_bytes = (size_t)1 << 30,
            size_t piece = 8u << 20)
      : ctx_(ctx), sink_(std::move(sink)), exclude_(exclude_flags), arena_bytes_(arena_bytes), ring_(4, piece) {
    if (!rfx_text_append_bgzf || !rfx_bam_header || !rfx_bam_settle || !rfx_bam_parse)
      die(tool_ + ": this library cannot read BAM input");
    for (rfx_text*& a : arena_) {
      a = rfx_text_open(ctx_, arena_bytes);
      if (!a) die(std::string("rufus_amd: rfx_text_open: ") + rfx_last_error());
    }
  }
  ~BamIngest() {
    ring_.settle_all();
    for (rfx_text* a : arena_) rfx_text_close(a);
  }
  // the other step per arena, and the tool the messages name (before feed_mapped)
  void set_per_arena(std::function<uint64_t(rfx_text*, uint64_t)> f, const std::string& tool) {
    per_arena_ = std::move(f);
    tool_ = tool;
  }
  // an arena's run list (rfx_bam_parse's ref_runs) stitched to the log: a run that begins an arena with the refID the arena
  // before ended with is no change
  void add_runs(const uint32_t* runs, uint64_t n_runs) {
    for (uint64_t i = 0; i < n_runs; ++i) {
      const int32_t ref = (int32_t)runs[2 * i + 1];
      if (chr_runs_.empty() || chr_runs_.back() != ref) chr_runs_.push_back(ref);
    }
  }
  // before feed_mapped, with ONE input: fd is the cache file, open for writing and empty
  void set_keep_packed(int fd, int min_q) {
    if (!rfx_bam_parse_filter || !rfx_bam_name_hashes || !rfx_bam_locate) die(tool_ + ": this library cannot keep a BAM's packed reads");
    cache_fd_ = fd;
    cache_minq_ = min_q;
  }
  // after feed_mapped: the block index and the header that makes the file a cache
  void finish_keep_packed() {
    if (cache_fd_ < 0) return;
    const bool ok = cache_.finish();
    if (::close(cache_fd_) != 0 || !ok) cache_write_error();
    cache_fd_ = -1;
  }
  std::string keep_counts() const {
    char b[200];
    snprintf(b, sizeof b, "bam cache: %llu records, %llu bytes, stream %llu bytes", (unsigned long long)cache_.records(),
             (unsigned long long)cache_.file_bytes(), (unsigned long long)cache_.stream_bytes());
    return b;
  }
  uint64_t reads() const { return reads_; }
  uint64_t records() const { return records_; }
  uint64_t arenas() const { return arenas_; }
  std::string counts() const {
    char b[200];
    snprintf(b, sizeof b, "bam route: %llu blocks in %llu appends, %llu arenas, %llu records, %llu reads", (unsigned long long)blocks_,
             (unsigned long long)appends_, (unsigned long long)arenas_, (unsigned long long)records_, (unsigned long long)reads_);
    if (!region_on_) return b;
    char r[200];
    snprintf(r, sizeof r, "; region tid %d [%lld, %lld) index %s: %llu blocks inflated, %llu records in the region", (int)region_.tid,
             (long long)region_.beg, (long long)region_.end, region_index_, (unsigned long long)blocks_, (unsigned long long)in_region_);
    return std::string(b) + r;
  }
  // PassThroughSamCheck's side file (src/PassThroughSamCheck.cpp:140-155): its initial `current`, then the RNAME of every
  // run of kept records in file order; refID -1 prints as `*`
  std::vector<std::string> chr_log() const {
    std::vector<std::string> out{"notachr"};
    for (int32_t ref : chr_runs_) out.push_back(ref < 0 || (size_t)ref >= ref_names_.size() ? std::string("*") : ref_names_[(size_t)ref]);
    return out;
  }

  // A whole mapped BAM file.  Dies on a header that is not BAM's, on a block that is not BGZF, not whole or does not
  // inflate, on a record rfx_bam_core.h refuses and on a file that ends inside a record.
  void feed_mapped(const char* m, size_t size) {
    int complete = 0;
    uint64_t names_bytes = 0, first_block = 0;
    uint32_t skip0 = 0;
    int rc = rfx_bam_header(m, size, &complete, &n_ref_, nullptr, 0, &names_bytes, &first_block, &skip0);
    if (rc == RFX_OK && complete) {
      std::vector<char> names((size_t)names_bytes + 1);
      rc = rfx_bam_header(m, size, &complete, &n_ref_, names.data(), names_bytes, &names_bytes, &first_block, &skip0);
      ref_names_.clear();
      for (size_t at = 0; at < (size_t)names_bytes; at += strlen(names.data() + at) + 1) ref_names_.emplace_back(names.data() + at);
    }
    if (rc != RFX_OK || !complete) die(tool_ + ": --bam: the input does not begin with a whole BAM header");
    // the cache's block index: EVERY block of the file from byte 0, the header's too (the stream is all of them); `base`:
    // the stream offset of the first arena's byte 0 = of the block the records begin in
    uint64_t base = 0;
    if (cache_fd_ >= 0) {
      std::string names;
      for (const std::string& n : ref_names_) names.append(n).push_back('\0');
      if (!cache_.open(cache_fd_, cache_minq_, exclude_, (uint32_t)n_ref_, names.data(), names.size())) cache_write_error();
      for (const BgzfRun& b : bgzf_runs(m, 0, size, 1u << 16, 1, tool_ + ": ", nullptr)) {  // (runs of one block)
        if (b.at == (size_t)first_block) base = cache_.stream_bytes();
        cache_.add_block((uint32_t)b.n, (uint32_t)b.inflated);
      }
    }
    // --region: the index's one range of blocks instead of all of them (region_range)
    bool ranged = false;
    uint64_t walk_from = first_block, walk_to = size, skip_first = skip0, stop_in = 0, stop_inf = 0;
    if (region_on_) {
      std::string why;
      if (!rfxbai::parse_region(region_text_, ref_names_, &region_, &why)) die(tool_ + ": --region: " + why);
      bool empty = false;
      ranged = region_range(m, size, first_block, skip0, &empty, &walk_from, &skip_first, &walk_to, &stop_in, &stop_inf);
      if (ranged && empty) return;  // no chunk: no arena, the outputs of an empty input
      if (!ranged) {
        walk_from = first_block;
        walk_to = size;
        skip_first = skip0;
      }
    }
    uint64_t range_inflated = 0;
    const std::vector<BgzfRun> runs = bgzf_runs(m, (size_t)walk_from, (size_t)walk_to, ring_.cap(), bgzf_run_blocks(arena_bytes_),
                                                tool_ + (per_arena_ ? ": --bam: " : ": "), &blocks_, &range_inflated);
    if (ranged && runs.empty()) return;
    // STOP as an offset in the inflated bytes of the range (the first arena's byte 0 = the first block's)
    const uint64_t stop_stream = stop_in ? range_inflated - stop_inf + stop_in : range_inflated;
    int cur = 0;
    size_t i = 0;
    // (no check for a run that no arena holds: an arena that fills with nothing ends below, in n_records == 0)
    auto fill = [&](rfx_text* a) { return bgzf_fill(ring_, a, m, runs, i, appends_); };
    uint64_t skip = skip_first;
    bool more = fill(arena_[cur]);
    while (more) {
      rfx_text* t = arena_[cur];
      rfx_text* nx = arena_[cur ^ 1];
      uint64_t carried = 0;
      const uint64_t n_records = settle(t, nx, skip, &carried);
      if (n_records == 0) die(tool_ + ": --bam: a record that is longer than an arena");
      skip = 0;
      const uint64_t cut = rfx_text_bytes(t);  // (the next arena begins with what lay behind it: its byte 0 is stream byte base + cut)
      more = fill(nx);  // queued, not waited for: the device inflates it beside this arena's count
      parse_and_sink(t, n_records, base);
      base += cut;
      cur ^= 1;
    }
    uint64_t carried = 0;
    if (ranged) {  // the tail goes to the other arena (empty: reset behind its last parse) and is dropped with it
      rfx_text* t = arena_[cur];
      rfx_text* nx = arena_[cur ^ 1];
      const uint64_t n_records = settle(t, nx, skip, &carried);
      if (carried && base + rfx_text_bytes(t) < stop_stream)
        die(tool_ + ": --bam: --region: the index's range ends inside a record that starts in front of its end");
      parse_and_sink(t, n_records, base);
      rfx_text_reset(nx);
      return;
    }
    const uint64_t n_records = settle(arena_[cur], nullptr, skip, &carried);  // (a tail: the file ends inside a record)
    parse_and_sink(arena_[cur], n_records, base);
  }
};

// ---- two bgzip'd mate files in lock step: inflated, parsed, filtered and the hit pairs' text gathered on the device -------
// Replaces `RUFUS.Filter HashList <(zcat A) <(zcat B) STUB ...` (runRufus.sh:974-977): the host reads the two files and
// writes the pulled records, nothing else.  Record i of A pairs with record i of B (src/RUFUS.Filter.cpp:165-173), but
// BGZF blocks end anywhere and the mates' lines differ in length, so two full arenas hold different numbers of whole
// records.  Two arenas per mate; one thread feeds (BgzfIngest's run rule), and a STEP is
//   fill A[cur], B[cur]                      until the next run does not fit or the file ends
//   R = min(records(A[cur]), records(B[cur]))                                              rfx_text_records
//   cut both behind record R, the rest moves to the front of A[cur ^ 1], B[cur ^ 1]        rfx_text_settle_records
//   fill A[cur ^ 1], B[cur ^ 1]              queued, not waited for: inflated beside what follows
//   parse both (RFX_PACK_FILTER), filter both, OR the two masks            (a pair is pulled when either mate was hit)
//   gather the OR'd records' text of both arenas into page-locked memory                  rfx_text_gather
//   hand the two runs of bytes to the sink, reset A[cur], B[cur], cur ^= 1
// Every step takes at least one record off both mates or ends the run, so the loop ends.
// The end of a file: one '\n' is appended behind its last run.  A file that ended with a newline then ends with one blank
// line, a file that did not ends as it should: what is left of mate 1 behind its last whole record must be that one byte
// or nothing -- anything else is a file that ends inside a record.  Mate 1 at its end ends the run (what mate 2 still
// holds is ignored, as src/RUFUS.Filter.cpp:165 stops at the end of file 1); mate 2 at its end with records of mate 1
// left is refused -- the text route's records of empty lines for the missing mates are not reproduced.
// (weak, as above: tests/host/filter_sam_harness.cpp links the executable's source against a stand-in without a text arena)
#pragma weak rfx_text_records
#pragma weak rfx_text_settle_records
#pragma weak rfx_text_gather
#pragma weak rfx_reads_of_length
class BgzfPairFilter {
 public:
  // (mate 1's bytes, mate 2's bytes, pairs of this step, pairs pulled)
  using Sink = std::function<void(const char*, size_t, const char*, size_t, uint64_t, uint64_t)>;

 private:
  rfx_ctx* ctx_;
  rfx_set* set_;
  int min_q_, thresh_;
  Sink sink_;
  uint64_t arena_bytes_;
  struct Mate {
    const char* m = nullptr;
    std::vector<BgzfRun> runs;
    size_t i = 0;         // the next run to queue
    bool closed = false;  // every run is queued and the final newline lies behind them
    rfx_text* arena[2] = {nullptr, nullptr};
    std::vector<uint64_t> mask;
    PinnedBuf out;  // the gathered text
  };
  Mate mate_[2];
  PinnedRing ring_;
  uint64_t blocks_ = 0, appends_ = 0, steps_ = 0, pairs_ = 0, pulled_ = 0;

  [[noreturn]] static void fail(const char* what, int rc) {
    if (rc == RFX_E_FORMAT && !strncmp(rfx_last_error(), "rfx_bgzf:", 9)) die(std::string("rufus_amd RUFUS.Filter: ") + rfx_last_error());
    die_rc(what, rc);
  }

  void reset(rfx_text* t) {
    ring_.settle_arena(t);
    rfx_text_reset(t);
  }
  // queues runs into arena `a` until the next does not fit or the file is at its end (then the newline behind it)
  void fill(Mate& M, rfx_text* a) {
    if (bgzf_fill(ring_, a, M.m, M.runs, M.i, appends_, fail)) return;
    if (!M.closed && rfx_text_room(a) >= 1) {
      static const char nl = '\n';
      const long tk = rfx_text_append(a, &nl, 1);
      if (tk < 0) fail("rfx_text_append", (int)tk);
      M.closed = true;
    }
  }
  uint64_t records(rfx_text* t) {
    uint64_t n = 0;
    const int rc = rfx_text_records(t, &n);
    if (rc != RFX_OK) fail("rfx_text_records", rc);
    return n;
  }
  void cut(rfx_text* t, rfx_text* next, uint64_t n) {
    uint64_t kept = 0, carried = 0;
    const int rc = rfx_text_settle_records(t, next, n, &kept, &carried);
    if (rc == RFX_E_RANGE) die_not_strict();  // (cannot be: the arenas of a mate are equally large)
    if (rc != RFX_OK) fail("rfx_text_settle_records", rc);
    if (kept != n) die("rufus_amd RUFUS.Filter: an arena lost records between the count and the cut");
  }
  void gather(Mate& M, rfx_text* t, const uint64_t* mask, uint64_t n, uint64_t* bytes, uint64_t* n_sel) {
    for (;;) {
      const int rc = rfx_text_gather(t, mask, n, M.out.p, M.out.cap, bytes, n_sel);
      if (rc == RFX_OK) return;
      if (rc != RFX_E_RANGE) fail("rfx_text_gather", rc);
      M.out.need((size_t)*bytes);
    }
  }

 public:
  BgzfPairFilter(rfx_ctx* ctx, rfx_set* set, int min_q, int thresh, Sink sink, size_t arena_bytes = (size_t)1 << 30,
                 size_t piece = 8u << 20)
      : ctx_(ctx), set_(set), min_q_(min_q), thresh_(thresh), sink_(std::move(sink)), arena_bytes_(arena_bytes), ring_(8, piece) {
    if (!rfx_text_open || !rfx_text_close || !rfx_text_room || !rfx_text_bytes || !rfx_text_append || !rfx_text_wait ||
        !rfx_text_reset || !rfx_text_parse || !rfx_text_append_bgzf || !rfx_text_records || !rfx_text_settle_records ||
        !rfx_text_gather || !rfx_reads_of_length)
      die("rufus_amd RUFUS.Filter: this library cannot inflate BGZF input");
    if (arena_bytes_ < 4 * 65536) die("rufus_amd RUFUS.Filter: RFX_FILTER_ARENA must be at least 262144 bytes");
    for (Mate& M : mate_)
      for (rfx_text*& a : M.arena) {
        a = rfx_text_open(ctx_, arena_bytes_);
        if (!a) die(std::string("rufus_amd: rfx_text_open: ") + rfx_last_error());
      }
  }
  ~BgzfPairFilter() {
    ring_.settle_all();
    for (Mate& M : mate_)
      for (rfx_text* a : M.arena) rfx_text_close(a);
  }
  std::string counts() const {
    char b[200];
    snprintf(b, sizeof b, "filter: bgzf route: %llu blocks in %llu appends, %llu steps, %llu pairs, %llu pulled",
             (unsigned long long)blocks_, (unsigned long long)appends_, (unsigned long long)steps_, (unsigned long long)pairs_,
             (unsigned long long)pulled_);
    return b;
  }
  uint64_t pairs() const { return pairs_; }
  uint64_t pulled() const { return pulled_; }

  // Two whole mapped BGZF files.  Dies on a block that is not BGZF, not whole or does not inflate, on text that is not
  // strict 4-line FASTQ, on an empty sequence line in mate 1 and on a mate 2 with fewer records than mate 1.
  void run(const char* m1, size_t n1, const char* m2, size_t n2) {
    mate_[0].m = m1;
    mate_[1].m = m2;
    const size_t sizes[2] = {n1, n2};
    for (int m = 0; m < 2; ++m)
      mate_[m].runs = bgzf_runs(mate_[m].m, 0, sizes[m], ring_.cap(), bgzf_run_blocks(arena_bytes_), "rufus_amd RUFUS.Filter: ", &blocks_);
    int cur = 0;
    for (Mate& M : mate_) fill(M, M.arena[cur]);
    for (;;) {
      rfx_text* t[2] = {mate_[0].arena[cur], mate_[1].arena[cur]};
      rfx_text* nx[2] = {mate_[0].arena[cur ^ 1], mate_[1].arena[cur ^ 1]};
      const uint64_t r1 = records(t[0]), r2 = records(t[1]);
      const uint64_t n = std::min(r1, r2);
      if (n == 0) {
        if (r1 == 0) {
          if (!mate_[0].closed || rfx_text_bytes(t[0]) > 1) die_not_strict();  // a full arena without a record / a file that ends inside one
          break;                                                               // mate 1 is at its end
        }
        if (!mate_[1].closed || rfx_text_bytes(t[1]) > 1) die_not_strict();
        die("rufus_amd RUFUS.Filter: mate files hold different numbers of records");
      }
      for (int m = 0; m < 2; ++m) cut(t[m], nx[m], n);
      for (int m = 0; m < 2; ++m) fill(mate_[m], nx[m]);  // queued, not waited for
      rfx_reads* rd[2] = {nullptr, nullptr};
      for (int m = 0; m < 2; ++m) {
        int strict = 1;
        rd[m] = rfx_text_parse(t[m], RFX_PACK_FILTER, min_q_, &strict);
        if (!rd[m] && !strict) die_not_strict();
        if (!rd[m]) fail("rfx_text_parse", RFX_E_HIP);
      }
      if (rfx_reads_of_length(rd[0], 0))
        die("rufus_amd RUFUS.Filter: empty sequence line (undefined behaviour in the reference) -- rejected");
      const size_t nw = (size_t)((n + 63) / 64);
      for (int m = 0; m < 2; ++m) {
        mate_[m].mask.assign(nw, 0);
        uint64_t nh = 0;
        // paired tool: `i < length()-1`, the last base is never examined (src/RUFUS.Filter.cpp:203)
        const int rc = rfx_filter(set_, rd[m], thresh_, 1, nullptr, mate_[m].mask.data(), &nh);
        if (rc) fail("rfx_filter", rc);
      }
      std::vector<uint64_t>& either = mate_[0].mask;  // == the reference's "mate 2 only if mate 1 failed" (:237-277)
      uint64_t any = 0;
      for (size_t w = 0; w < nw; ++w) {
        either[w] |= mate_[1].mask[w];
        if (w == nw - 1 && (n & 63)) either[w] &= (1ull << (n & 63)) - 1;
        any |= either[w];
      }
      uint64_t bytes[2] = {0, 0}, sel[2] = {0, 0};
      if (any)
        for (int m = 0; m < 2; ++m) gather(mate_[m], t[m], either.data(), n, &bytes[m], &sel[m]);
      if (sel[0] != sel[1]) die("rufus_amd RUFUS.Filter: the two mates' gathers disagree");
      sink_((const char*)mate_[0].out.p, (size_t)bytes[0], (const char*)mate_[1].out.p, (size_t)bytes[1], n, sel[0]);
      ++steps_;
      pairs_ += n;
      pulled_ += sel[0];
      for (int m = 0; m < 2; ++m) {
        rfx_reads_free(rd[m]);
        reset(t[m]);
      }
      cur ^= 1;
    }
  }
};

// ---- the subject's hit pairs straight from its BAM: two passes over the file, only selected records leave the device ----
// Replaces `samtools view -F 3328 X.bam | PassThroughSamCheck.stranded CHR STUB.temp | RUFUS.Filter ...`
// (runRufus.sh:964-967).  Mates of a coordinate-sorted BAM lie anywhere and hits are rare, so:
//   pass 1  BamIngest's walk; per arena rfx_bam_parse_filter -> rfx_filter (every record by itself, last base skipped) ->
//           rfx_bam_name_hashes of the hit records.  Kept: the hit records' GLOBAL kept indices (kept records in front of the
//           arena + index in it: the same however the arenas are cut), their name hashes, the refID runs for the log
//   between rfx_nameset_build of the hashes.  No hit: no second pass
//   pass 2  the same walk, no pack and no scan; per arena rfx_bam_mark_names -> rfx_bam_gather of the marked records
//   tail    rfx_bam_pairs.hpp: each gathered record printed as the stranded feeder prints it, its hit bit looked up by
//           global index, the pairing walk of `--sam` over this subset
// Exact: what becomes of a name depends only on the records of that name, and the subset holds every record of every hit
// name in stream order.  A hash collision brings records of a name without a hit: they pair among themselves and write
// nothing.
// (weak, as above)
#pragma weak rfx_bam_parse_filter
#pragma weak rfx_bam_name_hashes
#pragma weak rfx_nameset_build
#pragma weak rfx_nameset_size
#pragma weak rfx_nameset_free
#pragma weak rfx_bam_mark_names
#pragma weak rfx_bam_gather
#pragma weak rfx_reads_count
class BamPairFilter {
  rfx_ctx* ctx_;
  rfx_set* set_;
  int min_q_, thresh_;
  uint32_t exclude_;
  size_t arena_bytes_, piece_;
  std::vector<uint64_t> hit_index_, hit_hash_, mask_;  // (hit_index_ ascending: arenas come in file order)
  std::vector<uint32_t> runs_buf_;
  std::vector<std::string> chr_log_;
  std::vector<uint8_t> out_;
  rfxsam::BamPairTail tail_;
  uint64_t arenas_ = 0, records_ = 0, reads_ = 0, names_ = 0, passes_ = 0;
  std::string region_, bam_path_, ingest_counts_;  // set_region: both passes are BamIngest's ranged walk
  static constexpr const char* TOOL = "rufus_amd RUFUS.Filter";

  [[noreturn]] static void fail(const char* what) { die(std::string(TOOL) + ": --bam: " + what + ": " + rfx_last_error()); }

  uint64_t scan_arena(BamIngest& in, rfx_text* t, uint64_t n_records, uint64_t base) {
    runs_buf_.resize((size_t)2 * n_records);
    uint64_t n_runs = 0;
    rfx_reads* rd = rfx_bam_parse_filter(t, exclude_, min_q_, runs_buf_.data(), n_records, &n_runs);
    if (!rd) die(std::string(TOOL) + ": --bam: " + rfx_last_error());
    in.add_runs(runs_buf_.data(), n_runs);
    const uint64_t n = rfx_reads_count(rd);
    mask_.assign((size_t)((n + 63) / 64) + 1, 0);
    uint64_t nh = 0;
    // every record by itself; paired tool: `i < length()-1`, the last base is never examined (src/RUFUS.Filter.cpp:203)
    const int rc = rfx_filter(set_, rd, thresh_, 1, nullptr, mask_.data(), &nh);
    rfx_reads_free(rd);
    if (rc) fail("rfx_filter");
    if (nh) {
      const size_t at = hit_hash_.size();
      hit_hash_.resize(at + (size_t)nh);
      uint64_t got = 0;
      if (rfx_bam_name_hashes(t, exclude_, mask_.data(), n, hit_hash_.data() + at, nh, &got) != RFX_OK || got != nh)
        fail("rfx_bam_name_hashes");
      for (uint64_t i = 0; i < n; ++i)
        if ((mask_[i >> 6] >> (i & 63)) & 1) hit_index_.push_back(base + i);
    }
    return n;
  }
  uint64_t pull_arena(rfx_text* t, uint64_t n_records, uint64_t base, rfx_nameset* names) {
    mask_.assign((size_t)((n_records + 63) / 64) + 1, 0);
    uint64_t n_kept = 0, n_marked = 0;
    if (rfx_bam_mark_names(t, exclude_, names, mask_.data(), &n_kept, &n_marked) != RFX_OK) fail("rfx_bam_mark_names");
    if (!n_marked) return n_kept;
    uint64_t bytes = 0, sel = 0;
    int rc = rfx_bam_gather(t, exclude_, mask_.data(), n_kept, out_.data(), out_.size(), &bytes, &sel);
    if (rc == RFX_E_RANGE) {
      out_.resize((size_t)(bytes + bytes / 4 + 4096));
      rc = rfx_bam_gather(t, exclude_, mask_.data(), n_kept, out_.data(), out_.size(), &bytes, &sel);
    }
    if (rc != RFX_OK || sel != n_marked) fail("rfx_bam_gather");
    uint64_t p = 0;
    for (uint64_t i = 0; i < n_kept; ++i) {
      if (!((mask_[i >> 6] >> (i & 63)) & 1)) continue;
      // (the device copied whole records the settle has checked; the sizes are checked again before anything is read)
      if (p + BAM_FIXED > bytes || bam_next(out_.data(), p, bytes) == BAM_STOP || bam_valid(out_.data(), p, 0x7FFFFFFF) != BAM_OK)
        die(std::string(TOOL) + ": --bam: the gathered records do not add up");
      tail_.add(out_.data(), p, std::binary_search(hit_index_.begin(), hit_index_.end(), base + i));
      p = bam_next(out_.data(), p, bytes);
    }
    if (p != bytes) die(std::string(TOOL) + ": --bam: the gathered records do not add up");
    return n_kept;
  }
  void pass(const char* m, size_t size, rfx_nameset* names) {
    BamIngest in(ctx_, nullptr, exclude_, arena_bytes_, piece_);
    uint64_t base = 0;
    if (!region_.empty()) in.set_region(region_, bam_path_, /*quiet=*/names != nullptr);
    in.set_per_arena(
        [&](rfx_text* t, uint64_t n_records) {
          const uint64_t n = names ? pull_arena(t, n_records, base, names) : scan_arena(in, t, n_records, base);
          base += n;
          return n;
        },
        TOOL);
    in.feed_mapped(m, size);
    if (!names) {
      arenas_ = in.arenas();
      records_ = in.records();
      reads_ = in.reads();
      chr_log_ = in.chr_log();
      ingest_counts_ = in.counts();
    } else if (in.records() != records_ || in.reads() != reads_) {
      die(std::string(TOOL) + ": --bam: the two passes saw different records");
    }
    ++passes_;
  }

 public:
  BamPairFilter(rfx_ctx* ctx, rfx_set* set, int min_q, int thresh, uint32_t exclude_flags, size_t arena_bytes = (size_t)1 << 30,
                size_t piece = 8u << 20)
      : ctx_(ctx), set_(set), min_q_(min_q), thresh_(thresh), exclude_(exclude_flags), arena_bytes_(arena_bytes), piece_(piece) {
    if (!rfx_bam_parse_filter || !rfx_bam_name_hashes || !rfx_nameset_build || !rfx_nameset_size || !rfx_nameset_free ||
        !rfx_bam_mark_names || !rfx_bam_gather)
      die(std::string(TOOL) + ": this library cannot read BAM input");
  }
  // before run(): only the records that overlap the region take part -- in the scan, in the log and in the pairing by name,
  // as behind `samtools view X.bam REG`, where a mate outside the region never reaches the filter
  void set_region(const std::string& text, const std::string& bam_path) {
    region_ = text;
    bam_path_ = bam_path;
  }
  // A whole mapped BAM file.  Dies where BamIngest does.  Afterwards mate1() / mate2() hold the two output files' bytes and
  // chr_log() the chromosome log's lines.
  void run(const char* m, size_t size) {
    pass(m, size, nullptr);
    trace("filter --bam: pass 1 done (scan)");
    if (hit_index_.empty()) return;
    rfx_nameset* names = rfx_nameset_build(ctx_, hit_hash_.data(), hit_hash_.size());
    if (!names) fail("rfx_nameset_build");
    names_ = rfx_nameset_size(names);
    pass(m, size, names);
    rfx_nameset_free(names);
    trace("filter --bam: pass 2 done (pull)");
  }
  const std::string& mate1() const { return tail_.walk.o1; }
  const std::string& mate2() const { return tail_.walk.o2; }
  const std::vector<std::string>& chr_log() const { return chr_log_; }
  uint64_t passes() const { return passes_; }
  std::string counts() const {
    char b[240];
    snprintf(b, sizeof b, "bam filter route: arenas %llu records %llu reads %llu hits %llu names %llu gathered %llu pairs %llu",
             (unsigned long long)arenas_, (unsigned long long)records_, (unsigned long long)reads_,
             (unsigned long long)hit_index_.size(), (unsigned long long)names_, (unsigned long long)tail_.records,
             (unsigned long long)tail_.walk.n_found);
    return region_.empty() ? std::string(b) : std::string(b) + " | " + ingest_counts_;
  }
};

// ---- the subject's hit reads straight from a single-end BAM: one pass, on the device -------------------------------------
// Replaces `samtools view -F 3328 X.bam [REG] | PassThroughSamCheck.stranded.se CHR | RUFUS.Filter.single HashList stdin ...`
// (runRufus.sh:1031-1032).  Nothing is paired by name, so what becomes of a record depends on that record alone and ONE
// pass is exact: BamIngest's walk (the region and its .bai range are BamIngest's, unchanged), and per settled arena
//   rfx_bam_parse_filter(MinQ)    the stranded filter form; the refID runs stitched by BamIngest::add_runs
//   rfx_bam_gather_hits(thresh, last_base_skipped = 0)    src/RUFUS.Filter.ss.cpp:176-193 examines the last base; the
//                                 selected records' bytes and their counts into page-locked memory, which grows on
//                                 RFX_E_RANGE: one retry with the sizes the call reported
//   tail    rfx_bam_single.hpp: every gathered record checked, printed as the stranded feeder prints it, `:MH<hits>`
// The text goes to the sink arena by arena, in stream order; nothing is held for the whole file.
// (weak, as above)
#pragma weak rfx_bam_gather_hits
class BamSingleFilter {
  rfx_ctx* ctx_;
  rfx_set* set_;
  int min_q_, thresh_;
  uint32_t exclude_;
  size_t arena_bytes_, piece_;
  std::function<void(const char*, size_t)> sink_;
  std::vector<uint32_t> runs_buf_;
  std::vector<std::string> chr_log_;
  PinnedBuf out_, hits_;
  rfxsam::BamSingleTail tail_;
  uint64_t arenas_ = 0, records_ = 0, reads_ = 0;
  std::string region_, bam_path_, ingest_counts_;
  static constexpr const char* TOOL = "rufus_amd RUFUS.Filter.single";

  uint64_t arena_step(BamIngest& in, rfx_text* t, uint64_t n_records) {
    runs_buf_.resize((size_t)2 * n_records);
    uint64_t n_runs = 0;
    rfx_reads* rd = rfx_bam_parse_filter(t, exclude_, min_q_, runs_buf_.data(), n_records, &n_runs);
    if (!rd) die(std::string(TOOL) + ": --bam: " + rfx_last_error());
    in.add_runs(runs_buf_.data(), n_runs);
    const uint64_t n = rfx_reads_count(rd);
    uint64_t bytes = 0, sel = 0;
    auto pull = [&] {
      return rfx_bam_gather_hits(t, exclude_, set_, rd, thresh_, /*last_base_skipped=*/0, out_.p, out_.cap, &bytes, (uint32_t*)hits_.p,
                                 nullptr, hits_.cap / 4, &sel);
    };
    int rc = pull();
    if (rc == RFX_E_RANGE) {
      out_.need((size_t)bytes);
      hits_.need((size_t)sel * 4);
      rc = pull();
    }
    rfx_reads_free(rd);
    if (rc != RFX_OK) die(std::string(TOOL) + ": --bam: " + rfx_last_error());
    std::string why;
    tail_.out.clear();
    if (!tail_.add((const uint8_t*)out_.p, bytes, (const uint32_t*)hits_.p, sel, &why)) die(std::string(TOOL) + ": --bam: " + why);
    if (!tail_.out.empty()) sink_(tail_.out.data(), tail_.out.size());
    return n;
  }

 public:
  // sink: the next stretch of STUB.Mutations.fastq, in stream order
  BamSingleFilter(rfx_ctx* ctx, rfx_set* set, int min_q, int thresh, uint32_t exclude_flags, std::function<void(const char*, size_t)> sink,
                  size_t arena_bytes = (size_t)1 << 30, size_t piece = 8u << 20)
      : ctx_(ctx), set_(set), min_q_(min_q), thresh_(thresh), exclude_(exclude_flags), arena_bytes_(arena_bytes), piece_(piece),
        sink_(std::move(sink)) {
    if (!rfx_bam_parse_filter || !rfx_bam_gather_hits || !rfx_reads_count) die(std::string(TOOL) + ": this library cannot read BAM input");
    out_.need((size_t)1 << 20);
    hits_.need((size_t)1 << 14);
  }
  // before run(): only the records that overlap the region take part, as behind `samtools view X.bam REG`
  void set_region(const std::string& text, const std::string& bam_path) {
    region_ = text;
    bam_path_ = bam_path;
  }
  // A whole mapped BAM file.  Dies where BamIngest does.  Afterwards chr_log() holds the chromosome log's lines.
  void run(const char* m, size_t size) {
    BamIngest in(ctx_, nullptr, exclude_, arena_bytes_, piece_);
    if (!region_.empty()) in.set_region(region_, bam_path_);
    in.set_per_arena([&](rfx_text* t, uint64_t n_records) { return arena_step(in, t, n_records); }, TOOL);
    in.feed_mapped(m, size);
    arenas_ = in.arenas();
    records_ = in.records();
    reads_ = in.reads();
    chr_log_ = in.chr_log();
    ingest_counts_ = in.counts();
    trace("filter --bam: pass 1 done");
  }
  const std::vector<std::string>& chr_log() const { return chr_log_; }
  std::string counts() const {
    char b[240];
    snprintf(b, sizeof b, "bam single route: arenas %llu records %llu reads %llu selected %llu windows %llu", (unsigned long long)arenas_,
             (unsigned long long)records_, (unsigned long long)reads_, (unsigned long long)tail_.records, (unsigned long long)tail_.windows);
    return region_.empty() ? std::string(b) : std::string(b) + " | " + ingest_counts_;
  }
};

// ---- the subject's hit pairs from its BAM and the count's cache: no pass over the file ----------------------------------
// Replaces BamPairFilter's two passes (and with them the second and third inflate of the subject's file, runRufus.sh:964-967
// after scripts/RunJellyForRUFUS.sh:28-29) when `jellyfish count --bam .. --keep-packed CACHE` has left rfx_bam_cache.hpp's
// file:
//   scan    per chunk rfx_reads_upload -> rfx_filter (every record by itself, last base skipped): scan_arena's masks, from
//           the arrays the same rfx_bam_parse_filter made.  Kept: the hit records' global kept indices and name hashes
//   mark    rfx_nameset_build of the hit hashes; the chunks' hash arrays through rfx_nameset_mark -> the selected records
//           (global index, stream offset, bytes), ascending
//   fetch   rfxbamcache::plan_fetch -> per batch the listed BGZF blocks, copied one behind the other into a page-locked
//           ring, rfx_text_append_bgzf, rfx_bam_fetch of the batch's records
//   verify  every fetched record: whole, bam_valid, and its QNAME's hash the cached one -- else the cache does not
//           describe this file (false: the caller takes the two-pass route; nothing has been written)
//   tail    BamPairTail::add in stream order, the hit bit by global index: BamPairFilter's tail
// Exact for BamPairFilter's reason: what becomes of a name depends only on the records of that name, in stream order, and
// the selection is every kept record whose name hash is in the hit set.
// (weak, as above)
#pragma weak rfx_bam_fetch
#pragma weak rfx_nameset_mark
class BamCachePull {
  rfx_ctx* ctx_;
  rfx_set* set_;
  int thresh_;
  size_t arena_bytes_, piece_;
  std::vector<uint64_t> hit_index_, hit_hash_, mask_;
  std::vector<std::string> chr_log_;
  rfxsam::BamPairTail tail_;
  uint64_t chunks_ = 0, records_ = 0, names_ = 0, selected_ = 0, blocks_ = 0, index_blocks_ = 0, batches_ = 0;
  static constexpr const char* TOOL = "rufus_amd RUFUS.Filter";

  [[noreturn]] static void fail(const char* what) { die(std::string(TOOL) + ": --packed: " + what + ": " + rfx_last_error()); }

 public:
  BamCachePull(rfx_ctx* ctx, rfx_set* set, int thresh, size_t arena_bytes = (size_t)1 << 30, size_t piece = 8u << 20)
      : ctx_(ctx), set_(set), thresh_(thresh), arena_bytes_(arena_bytes), piece_(std::max<size_t>(piece, 1u << 16)) {
    if (!rfx_bam_fetch || !rfx_nameset_mark || !rfx_nameset_build || !rfx_nameset_free || !rfx_text_append_bgzf)
      die(std::string(TOOL) + ": this library cannot fetch BAM records");
  }
  // the scan, from the cache alone.  Afterwards hits() says whether pull() has anything to do
  void scan(const rfxbamcache::Cache& cache) {
    uint64_t base = 0;
    std::vector<int32_t> runs;
    for (const rfxbamcache::Chunk& v : cache.chunks) {
      rfx_reads* rd = rfx_reads_upload(ctx_, v.codes, nullptr, v.good, v.word_off, v.len, v.n);
      if (!rd) fail("rfx_reads_upload");
      mask_.assign(((size_t)v.n + 63) / 64 + 1, 0);
      uint64_t nh = 0;
      // every record by itself; paired tool: `i < length()-1`, the last base is never examined (src/RUFUS.Filter.cpp:203)
      const int rc = rfx_filter(set_, rd, thresh_, 1, nullptr, mask_.data(), &nh);
      rfx_reads_free(rd);
      if (rc) fail("rfx_filter");
      for (uint32_t i = 0; i < v.n && nh; ++i)
        if ((mask_[i >> 6] >> (i & 63)) & 1) {
          hit_index_.push_back(base + i);
          hit_hash_.push_back(v.hash[i]);
        }
      for (uint32_t r = 0; r < v.n_runs; ++r) {  // BamIngest::add_runs' rule: a chunk that begins with the refID the one
        const int32_t ref = (int32_t)v.runs[2 * r + 1];  // before ended with is no change
        if (runs.empty() || runs.back() != ref) runs.push_back(ref);
      }
      base += v.n;
      ++chunks_;
    }
    records_ = base;
    index_blocks_ = cache.h.n_blocks;
    chr_log_.assign(1, "notachr");
    for (const int32_t ref : runs) chr_log_.push_back(ref < 0 || (size_t)ref >= cache.names.size() ? std::string("*") : cache.names[(size_t)ref]);
  }
  bool hits() const { return !hit_index_.empty(); }
  // m[0, size): the mapped BAM the cache was made from.  false: it is not -- a fetched record is not the record the cache
  // describes.  Dies on a block that does not inflate.
  bool pull(const rfxbamcache::Cache& cache, const char* m, size_t size) {
    rfx_nameset* names = rfx_nameset_build(ctx_, hit_hash_.data(), hit_hash_.size());
    if (!names) fail("rfx_nameset_build");
    names_ = rfx_nameset_size(names);
    std::vector<rfxbamcache::Selected> sel;
    std::vector<uint64_t> sel_index, sel_hash;
    uint64_t base = 0;
    for (const rfxbamcache::Chunk& v : cache.chunks) {
      mask_.assign(((size_t)v.n + 63) / 64 + 1, 0);
      uint64_t marked = 0;
      if (rfx_nameset_mark(names, v.hash, v.n, mask_.data(), &marked) != RFX_OK) fail("rfx_nameset_mark");
      for (uint32_t i = 0; i < v.n && marked; ++i)
        if ((mask_[i >> 6] >> (i & 63)) & 1) {
          rfxbamcache::Selected s;
          s.stream_off = v.stream_off + v.start[i];
          s.bytes = v.rbytes[i];
          sel.push_back(s);
          sel_index.push_back(base + i);
          sel_hash.push_back(v.hash[i]);
        }
      base += v.n;
    }
    rfx_nameset_free(names);
    selected_ = sel.size();
    std::vector<rfxbamcache::Batch> plan;
    std::string err;
    if (!rfxbamcache::plan_fetch(cache.index, cache.h.n_blocks, cache.h.stream_bytes, sel, arena_bytes_, plan, &err))
      die(std::string(TOOL) + ": --packed: " + err + " (RFX_BAM_ARENA)");
    rfx_text* arena = rfx_text_open(ctx_, arena_bytes_);
    if (!arena) fail("rfx_text_open");
    PinnedRing ring(4, piece_);
    std::vector<uint8_t> out;
    std::vector<uint32_t> nbytes;
    bool same = true;
    for (const rfxbamcache::Batch& b : plan) {
      // the batch's blocks, one behind the other (blocks that are not neighbours in the file are each self-contained)
      size_t k = 0;
      while (k < b.block.size()) {
        PinnedRing::Buf& buf = ring.take();
        size_t used = 0;
        for (; k < b.block.size(); ++k) {
          const rfxbamcache::IndexEntry& e = cache.index[b.block[k]];
          if (e.file_off + e.csize > size) die(std::string(TOOL) + ": --packed: the block index lies outside the file");  // (sizes agree: checked)
          if (used + e.csize > piece_) break;
          memcpy(buf.p + used, m + e.file_off, e.csize);
          used += e.csize;
        }
        const long tk = rfx_text_append_bgzf(arena, buf.p, used);
        if (tk == RFX_E_FORMAT) { same = false; break; }  // (not whole BGZF blocks where the index says blocks are)
        if (tk < 0) die_rc("rfx_text_append_bgzf", (int)tk);
        PinnedRing::sent(buf, arena, tk);
      }
      blocks_ += b.block.size();
      ++batches_;
      uint64_t total = 0, got = 0;
      nbytes.resize(b.n);
      for (size_t i = 0; i < b.n; ++i) total += (nbytes[i] = sel[b.first + i].bytes);
      out.resize((size_t)total + 8);
      if (same) {
        const int rc = rfx_bam_fetch(arena, b.arena_off.data(), nbytes.data(), b.n, out.data(), total, &got);
        if (rc == RFX_E_FORMAT && !strncmp(rfx_last_error(), "rfx_bgzf:", 9)) die(std::string(TOOL) + ": --packed: " + rfx_last_error());
        if (rc == RFX_E_FORMAT) same = false;  // (an entry is no record: not the file the cache was made from)
        else if (rc != RFX_OK || got != total) fail("rfx_bam_fetch");
      }
      uint64_t p = 0;
      for (size_t i = 0; i < b.n && same; ++i) {
        if (bam_next(out.data(), p, total) != p + nbytes[i] || bam_valid(out.data(), p, 0x7FFFFFFF) != BAM_OK ||
            bam_name_hash(out.data(), p) != sel_hash[b.first + i]) {
          same = false;
          break;
        }
        tail_.add(out.data(), p, std::binary_search(hit_index_.begin(), hit_index_.end(), sel_index[b.first + i]));
        p += nbytes[i];
      }
      ring.settle_arena(arena);
      rfx_text_reset(arena);
      if (!same) break;
    }
    rfx_text_close(arena);  // (nothing of the ring is in flight: every batch ends in settle_arena)
    return same;
  }
  const std::string& mate1() const { return tail_.walk.o1; }
  const std::string& mate2() const { return tail_.walk.o2; }
  const std::vector<std::string>& chr_log() const { return chr_log_; }
  std::string counts() const {
    char b[320];
    snprintf(b, sizeof b, "bam cache route: chunks %llu records %llu hits %llu names %llu selected %llu blocks %llu of %llu batches %llu pairs %llu",
             (unsigned long long)chunks_, (unsigned long long)records_, (unsigned long long)hit_index_.size(), (unsigned long long)names_,
             (unsigned long long)selected_, (unsigned long long)blocks_, (unsigned long long)index_blocks_, (unsigned long long)batches_,
             (unsigned long long)tail_.walk.n_found);
    return b;
  }
};

}  // namespace rfxcli
