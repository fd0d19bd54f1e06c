// Drop-in RUFUS.Filter (paired) and RUFUS.Filter.single (-DRFX_SINGLE_END), same argv and outputs:
//   RUFUS.Filter        HashList Mate1.fq Mate2.fq STUB K MinQ HashCountThreshold Threads   (runRufus.sh:967)
//       -> STUB.Mutations.Mate1.fastq, STUB.Mutations.Mate2.fastq        src/RUFUS.Filter.cpp:28,:47-54
//   RUFUS.Filter.single HashList FQ|stdin STUB K MinQ HashCountThreshold Threads
//       -> STUB.Mutations.fastq with ":MH<hits>" appended to each header  src/RUFUS.Filter.ss.cpp:27,:43-49,:198
//   RUFUS.Filter --sam | --packed | --bam ...: the subject's SAM stream, its packed cache or its BAM file as the input
//       (not in the reference: namespaces samf and bamf below)
//   RUFUS.Filter.single --sam | --bam ...: the same two inputs for a single-end subject (runRufus.sh -se, :1031-1032):
//       every record by itself, STUB.Mutations.fastq with ":MH<hits>"; --packed stays paired-only
// The two mate files may be named pipes written in lock step by PassThroughSamCheck.stranded, so
// they are read interleaved, 4 lines each (src/RUFUS.Filter.cpp:165-173) -- never one file ahead.
// Pulled records are written in input order (the reference's order depends on OpenMP scheduling; at
// one thread it is input order too).  The scan itself runs in k_filter; no CPU fallback.
//
// Every route is parse(argc, argv, FilterArgs&) -- the usage line, the argument count -- and a body that takes the
// FilterArgs; a route that falls back to another calls that route's body with a changed copy.  What the bodies share
// (hash list, devices, staging memory, the scan step, the output files and the finish) stands once, in front of them; each
// body calls it in its own order, which is the order of its refusals.  main() only dispatches.
#include <condition_variable>
#include <deque>
#include <fstream>
#include <map>
#include <memory>
#include <mutex>

#include "rfx_cli.hpp"

using namespace rfxcli;

#include <unordered_set>

#include "rfx_sam.hpp"
#include "rfx_packed_cache.hpp"
#include "rfx_bam_cache.hpp"
#include "rfx_ingest.hpp"

// the two executables this source makes; everything below asks SINGLE, nothing else asks the preprocessor
#ifdef RFX_SINGLE_END
static constexpr int SINGLE = 1;
static const char* const TOOL = "rufus_amd RUFUS.Filter.single";
#else
static constexpr int SINGLE = 0;
static const char* const TOOL = "rufus_amd RUFUS.Filter";
#endif

// ---- what the routes share ---------------------------------------------------------------------------------------------
// One run of one route.  The strings are argv's (or a caller's that outlives the run).
struct FilterArgs {
  const char* cache = nullptr;     // --packed
  const char* chr = nullptr;       // the chromosome log (the flag routes)
  const char* hashlist = nullptr;
  const char* in1 = nullptr;       // mate 1 / the one FASTQ, the SAM stream, the spool, the BAM
  const char* in2 = nullptr;       // mate 2 (the paired text route)
  std::string stub;
  int k = 0, min_q = 0, thresh = 0, threads = 0;
  uint32_t exclude = 3328;         // --bam-exclude
  const char* region = nullptr;    // --region
  bool has_caller = false;         // this run's caller still has work to do (a temporary file to remove): no leave()
};
// CHRFILE HashList INPUT STUB K MinQ HashCountThreshold Threads, as the flag routes find them from v[0] on
static void positional(FilterArgs& a, char** v) {
  a.chr = v[0];
  a.hashlist = v[1];
  a.in1 = v[2];
  a.stub = v[3];
  a.k = atoi(v[4]);
  a.min_q = atoi(v[5]);
  a.thresh = atoi(v[6]);
  a.threads = atoi(v[7]);
}

// An input by name; the first `stdin_names` of "stdin", "/dev/stdin", "-" mean descriptor 0.  < 0: said so on stdout, and
// the caller returns 0 (the reference tools report on stdout and exit 0; the shell checks for empty outputs).
static int open_input(const char* path, int stdin_names) {
  static const char* const names[] = {"stdin", "/dev/stdin", "-"};
  for (int i = 0; i < stdin_names; ++i)
    if (strcmp(path, names[i]) == 0) return 0;
  const int fd = ::open(path, O_RDONLY);
  if (fd < 0) printf("Error, MutFile could not be opened");
  return fd;
}

// The hash list in two steps, because the routes open their inputs and outputs between them.  false: said so, return 0.
static bool read_hash_list(const char* path, std::string& text) {
  std::ifstream f(path, std::ios::binary);
  if (!f.is_open()) {
    printf("Error, ParentHashFile could not be opened");
    return false;
  }
  text.assign(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
  return true;
}
// -> the keys and one spare slot (size() - 1 keys).  `tool` names the executable where k is refused; `announce`: the
// reference's two lines (not wanted from a route whose inner run prints them).
static std::vector<uint64_t> load_keys(const std::string& text, int k, const std::string& tool, bool announce = true) {
  if (k < 1 || k > 32) die(tool + ": hash size must be 1..32");
  const long nk = rfx_hashlist_keys(text.data(), text.size(), k, SINGLE, nullptr, 0);
  if (nk < 0) die("rufus_amd: cannot parse the hash list");
  std::vector<uint64_t> keys((size_t)nk + 1);
  rfx_hashlist_keys(text.data(), text.size(), k, SINGLE, keys.data(), keys.size());
  if (announce) printf("\nDone Hash Files\n\t Mutations Hash size is %ld\n", nk);
  return keys;
}

// The devices of a run (RUFUS_GPUS; a route that needs exactly one says so in its own words before it opens them), the
// k-mer set on each, and a lock per device: uploads and scans of one device go one at a time.
struct Devices {
  std::vector<rfx_ctx*> ctxs;
  std::vector<rfx_set*> sets;
  std::vector<std::mutex> mu;
  size_t size() const { return ctxs.size(); }
  void open(const std::vector<int>& gpus, const std::vector<uint64_t>& keys, int k, const char* traced) {
    ctxs = open_ctxs(gpus);
    for (rfx_ctx* c : ctxs) {
      rfx_set* st = rfx_set_build(c, keys.data(), (uint64_t)keys.size() - 1, k);
      if (!st) die(std::string("rufus_amd: ") + rfx_last_error());
      sets.push_back(st);
    }
    mu = std::vector<std::mutex>(ctxs.size());
    trace(traced);
  }
  // One packed block through device d: up, scanned, freed.  The paired tool never examines a read's last base
  // (`i < length()-1`, src/RUFUS.Filter.cpp:203) and wants the hit bit per read (`mask`); the single-end tool examines it
  // and wants the counts too (`hits`, else null; src/RUFUS.Filter.ss.cpp:176-198).
  void scan_block(size_t d, const uint64_t* codes, const uint32_t* good, const uint32_t* woff, const uint32_t* lens, uint32_t n,
                  int thresh, uint32_t* hits, uint64_t* mask) {
    std::lock_guard<std::mutex> g(mu[d]);
    rfx_reads* rd = rfx_reads_upload(ctxs[d], codes, nullptr, good, woff, lens, n);
    if (!rd) die(std::string("rufus_amd: upload failed: ") + rfx_last_error());
    uint64_t nh = 0;
    const int rc = rfx_filter(sets[d], rd, thresh, SINGLE ? 0 : 1, hits, mask, &nh);
    rfx_reads_free(rd);
    if (rc) die(std::string("rufus_amd: filter failed: ") + rfx_last_error());
  }
  void close() {
    for (rfx_set* st : sets) rfx_set_free(st);
    for (rfx_ctx* c : ctxs) rfx_close(c);
  }
};

// Packed reads go up from page-locked memory (a pageable source costs a staging copy inside the runtime, under the
// device lock).  A buffer asked for while the device is still being opened is plain memory, page-locked by lock() before
// its first upload.  (rfx_ingest.hpp's PinnedBuf grows by another rule and stays what it is.)
struct Pinned {
  void* p = nullptr;
  size_t cap = 0;
  bool locked = false;
  void* need(size_t bytes, bool device_up) {  // null: no memory
    if (bytes > cap) {
      if (p) rfx_host_free(p);
      cap = bytes + bytes / 4;
      p = device_up ? rfx_host_alloc(cap) : rfx_host_alloc_lazy(cap);
      locked = device_up;
    }
    return p;
  }
  void lock() {
    if (p && !locked) (void)rfx_host_pin(p);  // (refused: the upload stages the pageable buffer itself)
    locked = true;
  }
  ~Pinned() { if (p) rfx_host_free(p); }
};
// the four arrays of a packed block of n reads in `words` words, as rfx_pack_spans fills and scan_block uploads them
struct Staging {
  Pinned pin[4];
  uint64_t* codes = nullptr;
  uint32_t *good = nullptr, *woff = nullptr, *lens = nullptr;
  bool need(uint64_t words, size_t n, bool device_up = true) {  // false: no memory (the caller refuses, in its own way)
    codes = (uint64_t*)pin[0].need((words + 1) * 8, device_up);
    good = (uint32_t*)pin[1].need((words + 1) * 4, device_up);
    woff = (uint32_t*)pin[2].need((n + 1) * 4, device_up);
    lens = (uint32_t*)pin[3].need((n + 1) * 4, device_up);
    return codes && good && woff && lens;
  }
  void lock() {
    for (Pinned& b : pin) b.lock();
  }
};
static const char* const NO_STAGING = "rufus_amd: cannot allocate pinned staging memory";

// What a run writes: the chromosome log (the flag routes) and STUB.Mutations.Mate1.fastq / .Mate2.fastq, or
// STUB.Mutations.fastq alone: the single-end tool never opens out2, and what is written to it goes nowhere.
struct Outputs {
  FILE* chr = nullptr;
  std::ofstream out1, out2;
  bool open(const char* chr_path, const std::string& stub) {  // false: said so, return 0
    if (chr_path) chr = fopen(chr_path, "w");
    out1.open((stub + (SINGLE ? ".Mutations.fastq" : ".Mutations.Mate1.fastq")).c_str(), std::ios::binary);
    if (!SINGLE) out2.open((stub + ".Mutations.Mate2.fastq").c_str(), std::ios::binary);
    if ((chr_path && !chr) || !out1.is_open() || (!SINGLE && !out2.is_open())) {
      printf("ERROR, Output file could not be opened -%s\n", stub.c_str());
      return false;
    }
    return true;
  }
  // The end of a run: what is still to be written (the log's lines, the mates' text; each may be empty), everything
  // closed, the route's counts to the trace, the reference's last line, and the process leaves (rfx_cli.hpp leave():
  // unmapping 20 GB of input, unpinning the staging blocks and the runtime's own teardown took 0.5 s of a 1.5 s run) --
  // unless RFX_CLEAN_EXIT=1 asks for the orderly way, or the run has a caller: then the route's teardown follows.
  void finish(const std::vector<std::string>& chr_log, const std::string& mate1, const std::string& mate2, const std::string& counts,
              bool has_caller = false) {
    if (chr) {
      for (const std::string& name : chr_log) fprintf(chr, "%s\n", name.c_str());
      fclose(chr);
    }
    out1.write(mate1.data(), (std::streamsize)mate1.size());
    out2.write(mate2.data(), (std::streamsize)mate2.size());
    out1.close();
    out2.close();
    if (!counts.empty()) trace(counts.c_str());
    printf("\nDone running RUFUS.Filter.cpp\n");
    if (!has_caller) leave(0);
  }
};

// ---- RUFUS.Filter HashList A.fastq.gz B.fastq.gz STUB K MinQ HashCountThreshold Threads --------------------------------
// Both mate files bgzip'd (regular files whose first block rfx_bgzf_scan accepts): replaces runRufus.sh:974-977's
// `<(zcat A) <(zcat B)`.  The files are mapped and handed to rfx_ingest.hpp's BgzfPairFilter: inflated, parsed, scanned
// and the pulled pairs' text gathered on the device; this thread reads the files and appends what comes back to
// STUB.Mutations.Mate1.fastq / .Mate2.fastq, in input order.  RFX_FILTER_ARENA: bytes of text per arena (four arenas).
// Paired only; the text route (below) sends it here.
namespace bgzff {
static int run(const FilterArgs& a, int fd1, int fd2, const std::vector<uint64_t>& keys, Outputs& out) {
  const std::vector<int> gpus = gpu_list();
  if (gpus.size() != 1)
    die("rufus_amd RUFUS.Filter: BGZF input is inflated on the device, which needs one device (RUFUS_GPUS names more): "
        "inflate it and pipe it in");
  Devices dv;
  dv.open(gpus, keys, a.k, "filter: device open, set built");
  Mapped map[2];
  for (int m = 0; m < 2; ++m) {
    map[m] = map_regular(m ? fd2 : fd1, true);
    if (!map[m].ok) die(std::string("rufus_amd RUFUS.Filter: cannot map a mate file: ") + strerror(errno));
  }
  const size_t arena = env_arena("RFX_FILTER_ARENA", 0), piece = env_piece((size_t)8 << 20);  // (the route refuses an arena below 256 KiB)
  unsigned long long total = 0, found = 0;
  {
    BgzfPairFilter route(
        dv.ctxs[0], dv.sets[0], a.min_q, a.thresh,
        [&](const char* t1, size_t n1, const char* t2, size_t n2, uint64_t pairs, uint64_t pulled) {
          out.out1.write(t1, (std::streamsize)n1);
          out.out2.write(t2, (std::streamsize)n2);
          total += pairs;
          found += pulled;
          printf("Read in %llu lines: Found %llu \r", total * 4, found);
        },
        arena, piece);
    trace("filter: bgzf route, text arenas open");
    route.run(map[0].p, map[0].n, map[1].p, map[1].n);
    trace(route.counts().c_str());
    trace("filter: all pieces written");
    out.finish({}, "", "", "");
  }
  dv.close();
  return 0;
}
}  // namespace bgzff

// ---- RUFUS.Filter --sam CHRFILE HashList SAM|stdin STUB K MinQ HashCountThreshold Threads -----------------------------
// SURVEY row N1, filter half.  runRufus.sh:964-967 runs `generator | PassThroughSamCheck.stranded CHR STUB.temp` into two
// named pipes that RUFUS.Filter reads in lock step: SAM text -> pairing by QNAME -> FASTQ text -> two pipes -> parsed
// again -> packed.  Here the SAM stream is the filter's own input: helper threads find the fields of every line, put
// reverse-strand records back the way the feeder prints them (src/PassThroughSamCheck.stranded.cpp:188-223: reverse
// complement, bases other than ACGTN vanish, quality reversed), pack bases + quality mask and run the scan on EVERY
// record by itself (k_filter; `i < length()-1` as the paired tool, src/RUFUS.Filter.cpp:203); one thread then walks
// the pieces in stream order, writes the chromosome log (CHRFILE: "notachr", then the previous RNAME at every change)
// and pairs the records by name as the feeder does -- a record meets its waiting mate or waits -- and a pair one of
// whose records was hit is written: the LATER record to STUB.Mutations.Mate1.fastq, the stored one to Mate2, in the
// order the pairs complete.  The same bytes as the two-process route; no FASTQ text exists for the other pairs.
// A waiting record is a pointer into its piece (no copy); a piece is recycled LAG pieces later, and only the few
// records that still wait then (mates far apart, unpaired reads) are copied out.
//
// RUFUS.Filter.single --sam (the same arguments): the same pipeline -- reader, helper threads, the stranded form packed
// per record, the chromosome log -- for what `PassThroughSamCheck.stranded.se CHR | RUFUS.Filter.single HashList stdin ...`
// does with the stream (runRufus.sh:1031-1032; a CRAM subject, :609, gets one process instead of two).  The scan examines
// the last base too (`i < length()`, src/RUFUS.Filter.ss.cpp:176) and the counts come back; there is no pairing: the
// records whose count reaches the threshold are written in stream order to STUB.Mutations.fastq with ":MH<hits>" (:194-203).
namespace samf {
using namespace rfxsam;

// Where the printed forms of a piece's records go (reverse strand: bases and qualities again; a quality string shorter
// than its read: a padded copy): blocks taken as they are needed and kept for the next piece -- most records are
// forward-strand and need none.  (Until round 4 every piece buffer had room for the worst case behind its lines,
// zero-filled by vector::resize: 96 MB touched per 32 MB piece, 8 GB at Threads = 40.)
struct SideArena {
  static constexpr size_t BLOCK = (size_t)4 << 20;
  std::vector<std::pair<std::unique_ptr<char[]>, size_t>> blocks;
  size_t cur = 0, used = 0;
  void reset() { cur = used = 0; }
  char* take(size_t n) {  // n bytes that stay where they are until the next reset()
    while (cur < blocks.size() && used + n > blocks[cur].second) {
      ++cur;
      used = 0;
    }
    if (cur == blocks.size()) {
      const size_t cap = std::max(BLOCK, n);
      blocks.emplace_back(std::unique_ptr<char[]>(new char[cap]), cap);
      used = 0;
    }
    char* p = blocks[cur].first.get() + used;
    used += n;
    return p;
  }
};
struct SPiece {
  std::vector<char> text;  // [0, size): SAM lines (pipe route)
  size_t size = 0;
  const char* mapped = nullptr;  // a regular input file: the lines lie in its mapping
  SideArena side;               // the printed form of reverse-strand records
  std::vector<Rec> recs;
  std::vector<std::string> chr_runs;
  std::vector<uint64_t> mask;  // hit bit per record
  std::vector<uint32_t> hits;  // RUFUS.Filter.single: hit windows per record
  std::vector<uint32_t> waited;  // records of this piece that went into the waiting table
  uint64_t seq = 0;
};

static const char* const USAGE = "Call is --sam CHRFILE PreBuiltMutHash SAM|stdin firstpassfile hashsize MinQ HashCountThreshold threads\n";
static bool parse(int argc, char** argv, FilterArgs& a) {
  fputs(USAGE, stdout);
  if (argc < 10) {
    printf("ERROR: expected 9 arguments\n");
    return false;
  }
  positional(a, argv + 2);
  return true;
}

static int run(const FilterArgs& a) {
  const int min_q = a.min_q, thresh = a.thresh;
  std::string text;
  if (!read_hash_list(a.hashlist, text)) return 0;
  const int fd = open_input(a.in1, 3);
  if (fd < 0) return 0;
  Outputs out;
  if (!out.open(a.chr, a.stub)) return 0;
  const std::vector<uint64_t> keys = load_keys(text, a.k, TOOL);
  // RUFUS_GPUS: the pieces are dealt to the devices by helper thread (the filter shards by read block)
  Devices dv;
  dv.open(gpu_list(), keys, a.k, "filter --sam: device open, set built");
  const unsigned n_gpu = (unsigned)dv.size();
#ifdef F_SETPIPE_SZ
  (void)fcntl(fd, F_SETPIPE_SZ, 1 << 20);
#endif

  unsigned helpers = (unsigned)std::max(1, a.threads);
  helpers = std::min(helpers, rfx_host_cpus() > 2 ? rfx_host_cpus() - 2 : 1u);
  if (const char* ev = getenv("RFX_HOST_THREADS")) helpers = (unsigned)std::max(1, atoi(ev));
  helpers = std::max(helpers, n_gpu);
  const size_t PIECE = env_piece(32u << 20);
  const size_t LAG = 3;
  const size_t MAX_IN_FLIGHT = 2 * (size_t)helpers + 2 + LAG;

  std::mutex mu;
  std::condition_variable cv;
  std::deque<SPiece*> todo, spare;
  std::map<uint64_t, SPiece*> done;
  bool input_end = false;
  uint64_t n_pieces = 0;
  size_t in_flight = 0;
  // A regular file (the spool `jellyfish count --spool` left, a SAM file): mapped and cut at line ends, no copy -- one
  // reader thread copying out of the page cache gave 5.8 GB/s, less than the helpers parse.
  Mapped file;
  if (fd != 0 && !getenv("RFX_FILTER_NO_MMAP")) file = map_regular(fd, true);
  const char* map = file.p;
  const size_t map_size = file.n;
  std::thread reader([&] {
    if (map) {
      size_t at = 0;
      while (at < map_size) {
        size_t end = std::min(map_size, at + PIECE);
        if (end < map_size) {
          const char* nl = (const char*)memchr(map + end, '\n', map_size - end);
          end = nl ? (size_t)(nl - map) + 1 : map_size;
        }
        SPiece* pc = nullptr;
        {
          std::unique_lock<std::mutex> g(mu);
          cv.wait(g, [&] { return in_flight < MAX_IN_FLIGHT; });
          if (!spare.empty()) { pc = spare.front(); spare.pop_front(); }
          ++in_flight;
        }
        if (!pc) pc = new SPiece();
        pc->mapped = map + at;
        pc->size = end - at;
        at = end;
        std::lock_guard<std::mutex> g(mu);
        pc->seq = n_pieces++;
        todo.push_back(pc);
        cv.notify_all();
      }
      std::lock_guard<std::mutex> g(mu);
      input_end = true;
      cv.notify_all();
      return;
    }
    std::vector<char> carry;
    bool eof = false;
    while (!eof) {
      SPiece* pc = nullptr;
      {
        std::unique_lock<std::mutex> g(mu);
        cv.wait(g, [&] { return in_flight < MAX_IN_FLIGHT; });
        if (!spare.empty()) { pc = spare.front(); spare.pop_front(); }
        ++in_flight;
      }
      if (!pc) pc = new SPiece();
      pc->mapped = nullptr;
      size_t fill = carry.size();
      if (pc->text.size() < fill + PIECE + (1u << 20)) pc->text.resize(fill + PIECE + (1u << 20));
      if (fill) memcpy(pc->text.data(), carry.data(), fill);  // (an empty vector may hand out a null pointer)
      carry.clear();
      bool have_nl = fill && memchr(pc->text.data(), '\n', fill);
      while (fill < PIECE || !have_nl) {  // at least PIECE bytes AND one line end
        if (fill == pc->text.size()) pc->text.resize(fill * 2);
        const size_t room = pc->text.size() - fill, want_more = fill < PIECE ? PIECE + (1u << 20) - fill : (size_t)1 << 20;
        const ssize_t n = ::read(fd, pc->text.data() + fill, std::min(room, want_more));
        if (n < 0 && errno == EINTR) continue;
        if (n < 0) die(std::string("read error on input: ") + strerror(errno));
        if (n == 0) { eof = true; break; }
        if (!have_nl && memchr(pc->text.data() + fill, '\n', (size_t)n)) have_nl = true;
        fill += (size_t)n;
      }
      size_t cut = fill;
      if (!eof) {
        while (cut > 0 && pc->text[cut - 1] != '\n') --cut;
        carry.assign(pc->text.data() + cut, pc->text.data() + fill);
      }
      pc->size = cut;
      std::lock_guard<std::mutex> g(mu);
      pc->seq = n_pieces++;
      todo.push_back(pc);
      cv.notify_all();
    }
    std::lock_guard<std::mutex> g(mu);
    input_end = true;
    cv.notify_all();
  });

  auto helper = [&](unsigned me) {
    const size_t dev = (size_t)me % (size_t)n_gpu;
    Staging stage;
    std::vector<uint64_t> so, qo;
    std::vector<uint32_t> sl;
    std::string rs, rq;
    Field f[11];
    for (;;) {
      SPiece* pcp;
      {
        std::unique_lock<std::mutex> g(mu);
        cv.wait(g, [&] { return !todo.empty() || input_end; });
        if (todo.empty()) return;
        pcp = todo.front();
        todo.pop_front();
      }
      SPiece& pc = *pcp;
      pc.recs.clear();
      pc.chr_runs.clear();
      pc.waited.clear();
      // (offsets handed to rfx_pack_spans are byte distances from `base`, modulo 2^64: the printed forms lie in other
      // allocations than the lines)
      const char* base = pc.mapped ? pc.mapped : pc.text.data();
      const char *p = base, *e = base + pc.size;
      pc.side.reset();
      const char* cur = nullptr;
      size_t cur_len = 0;
      uint64_t words = 0;
      while (p < e) {
        const char* nl = find_nl(p, e);
        const char* le = nl ? nl : e;
        if (split_sam(p, le, f)) {  // fewer than 11 fields: skipped, as the feeders do
          if (!cur || f[2].n != cur_len || memcmp(f[2].p, cur, cur_len) != 0) {
            pc.chr_runs.emplace_back(f[2].p, f[2].n);
            cur = f[2].p;
            cur_len = f[2].n;
          }
          Rec r;
          r.name = f[0].p; r.name_len = (uint32_t)f[0].n;
          r.seq = f[9].p; r.seq_len = (uint32_t)f[9].n;
          r.qual = f[10].p; r.qual_len = (uint32_t)f[10].n;
          if (sam_flag(f[1]) & 16) {
            revcomp_into(rs, f[9]);
            reverse_into(rq, f[10]);
            char* side = pc.side.take(rs.size() + rq.size());
            memcpy(side, rs.data(), rs.size());
            memcpy(side + rs.size(), rq.data(), rq.size());
            r.seq = side; r.seq_len = (uint32_t)rs.size();
            r.qual = side + rs.size(); r.qual_len = (uint32_t)rq.size();
          }
          r.hash = name_hash(r.name, r.name_len);
          words += (r.seq_len + 31) / 32;
          pc.recs.push_back(r);
        }
        p = nl ? nl + 1 : e;
      }
      const size_t n = pc.recs.size();
      pc.mask.assign((n + 63) / 64, 0);
      if (SINGLE) pc.hits.assign(n, 0);
      if (n) {
        so.resize(n); qo.resize(n); sl.resize(n);
        for (size_t i = 0; i < n; ++i) {
          const Rec& r = pc.recs[i];
          so[i] = (uint64_t)((uintptr_t)r.seq - (uintptr_t)base);
          sl[i] = r.seq_len;
          if (r.qual_len >= r.seq_len) {
            qo[i] = (uint64_t)((uintptr_t)r.qual - (uintptr_t)base);
          } else {  // a quality string shorter than its read: the missing characters are bad ('\0'), as in the file route
            char* side = pc.side.take(r.seq_len);
            memcpy(side, r.qual, r.qual_len);
            memset(side + r.qual_len, 0, r.seq_len - r.qual_len);
            qo[i] = (uint64_t)((uintptr_t)side - (uintptr_t)base);
          }
        }
        if (!stage.need(words, n)) die(NO_STAGING);
        stage.woff[0] = 0;
        if (rfx_pack_spans(base, so.data(), sl.data(), qo.data(), (uint32_t)n, min_q, RFX_PACK_FILTER, stage.codes, nullptr,
                           stage.good, stage.woff, stage.lens) != RFX_OK)
          die("rufus_amd: pack failed");
        dv.scan_block(dev, stage.codes, stage.good, stage.woff, stage.lens, (uint32_t)n, thresh,
                      SINGLE ? pc.hits.data() : nullptr, pc.mask.data());
      }
      std::lock_guard<std::mutex> g(mu);
      done[pc.seq] = pcp;
      cv.notify_all();
    }
  };
  std::vector<std::thread> workers;
  for (unsigned t = 0; t < helpers; ++t) workers.emplace_back(helper, t);

  PairWalk walk;  // (rfx_sam.hpp: the walk `--bam` runs too)
  WaitTable& waiting = walk.waiting;
  std::string &o1 = walk.o1, &o2 = walk.o2;
  unsigned long long &n_pairs = walk.n_pairs, &n_found = walk.n_found;
  std::deque<SPiece*> live;
  std::string current = "notachr";
  unsigned long long n_rec = 0;
  auto retire = [&](SPiece* pc) {  // what still waits from this piece leaves it
    for (uint32_t idx : pc->waited) {
      const Rec* r = &pc->recs[idx];
      const long at = waiting.find(r->hash, r->name, r->name_len);
      if (at < 0 || waiting.slot[(size_t)at].rec != r) continue;
      Owned* o = new Owned();
      o->bytes.assign(r->name, r->name_len);
      o->bytes.append(r->seq, r->seq_len);
      o->bytes.append(r->qual, r->qual_len);
      o->r = *r;
      o->r.name = o->bytes.data();
      o->r.seq = o->bytes.data() + r->name_len;
      o->r.qual = o->bytes.data() + r->name_len + r->seq_len;
      waiting.slot[(size_t)at].rec = &o->r;
      waiting.slot[(size_t)at].owned = o;
    }
    std::lock_guard<std::mutex> g(mu);
    spare.push_back(pc);
    --in_flight;
    cv.notify_all();
  };
  for (uint64_t want = 0;; ++want) {
    SPiece* pc;
    {
      std::unique_lock<std::mutex> g(mu);
      cv.wait(g, [&] { return done.count(want) || (input_end && want >= n_pieces); });
      if (!done.count(want)) break;
      pc = done[want];
      done.erase(want);
    }
    for (const std::string& name : pc->chr_runs)
      if (name != current) {
        fprintf(out.chr, "%s\n", current.c_str());
        current = name;
      }
    const size_t n = pc->recs.size();
    for (size_t i = 0; i < n; ++i) {
      const Rec& r = pc->recs[i];
      if (!SINGLE) {
        const uint32_t hit = (uint32_t)((pc->mask[i >> 6] >> (i & 63)) & 1);
        if (walk.meet(r, hit)) pc->waited.push_back((uint32_t)i);
        continue;
      }
      // no pairing: a record whose count reaches the threshold is written, `@QNAME:MH<hits>` (selected by the COUNT, as the
      // reference's `>=` does: a threshold <= 0 writes every record)
      ++n_pairs;
      if ((int)pc->hits[i] < thresh) continue;
      ++n_found;
      o1.push_back('@');
      o1.append(r.name, r.name_len);
      o1.append(":MH").append(std::to_string(pc->hits[i])).push_back('\n');
      o1.append(r.seq, r.seq_len);
      o1.append("\n+\n", 3);
      o1.append(r.qual, r.qual_len);
      o1.push_back('\n');
    }
    n_rec += n;
    if (!o1.empty()) {
      out.out1.write(o1.data(), (std::streamsize)o1.size());
      out.out2.write(o2.data(), (std::streamsize)o2.size());
      o1.clear();
      o2.clear();
    }
    live.push_back(pc);
    if (live.size() > LAG) {
      retire(live.front());
      live.pop_front();
    }
    printf("Read in %llu lines: Found %llu \r", n_pairs * 4, n_found);
  }
  while (!live.empty()) {
    retire(live.front());
    live.pop_front();
  }
  reader.join();
  for (auto& w : workers) w.join();
  trace("filter --sam: all pieces done");
  printf("\nSAM records %llu, pairs %llu, pulled %llu\n", n_rec, n_pairs, n_found);
  out.finish({current}, "", "", "", a.has_caller);
  dv.close();
  return 0;
}
}  // namespace samf

// ---- RUFUS.Filter --bam CHRFILE HashList X.bam STUB K MinQ HashCountThreshold Threads [--bam-exclude N] ---------------
// The subject straight from its BAM: what `samtools view -F N X.bam | RUFUS.Filter --sam CHRFILE HashList stdin ...` writes
// (runRufus.sh:964-967; N defaults to 3328), byte for byte, without samtools and without SAM text.  The file is mapped and
// handed to rfx_ingest.hpp's BamPairFilter: two passes, inflated and framed on the device both times; this thread reads
// the file and writes the three outputs.  One device: RUFUS_GPUS naming more is refused, as for the bgzip'd mates.
// RFX_BAM_ARENA (bytes per arena, >= 1 MiB) and RFX_INGEST_PIECE as in `jellyfish count --bam`.  Threads is accepted and
// not used: no host thread parses anything.
//
// RUFUS.Filter.single --bam ...: the same arguments, checks and refusals; what `samtools view -F N X.bam
// [REG] | PassThroughSamCheck.stranded.se CHRFILE | RUFUS.Filter.single HashList stdin STUB K MinQ Threshold 1` writes
// (runRufus.sh:1031-1032), byte for byte: STUB.Mutations.fastq and CHRFILE.  rfx_ingest.hpp's BamSingleFilter: ONE pass --
// nothing is paired by name -- and the file's text is written arena by arena, in stream order.
namespace bamf {
static const char* const USAGE =
    "Call is --bam CHRFILE PreBuiltMutHash X.bam firstpassfile hashsize MinQ HashCountThreshold threads [--bam-exclude N] [--region REG]\n";
static bool parse(int argc, char** argv, FilterArgs& a) {
  fputs(USAGE, stdout);
  if (argc < 10) {
    printf("ERROR: expected 9 arguments\n");
    return false;
  }
  positional(a, argv + 2);
  // --region REG: `samtools view -F N X.bam REG` in front of both passes (BamIngest::set_region)
  for (int i = 10; i < argc; ++i) {
    if (strcmp(argv[i], "--bam-exclude") == 0 && i + 1 < argc) a.exclude = (uint32_t)strtoul(argv[++i], nullptr, 0);
    else if (strcmp(argv[i], "--region") == 0 && i + 1 < argc) {
      if (a.region) die(std::string(TOOL) + ": --bam: --region given twice: one region per run");
      a.region = argv[++i];
    } else die(std::string(TOOL) + ": --bam: unknown argument " + argv[i]);
  }
  return true;
}

static int run(const FilterArgs& a) {
  std::string text;
  if (!read_hash_list(a.hashlist, text)) return 0;
  const int fd = open_input(a.in1, 0);
  if (fd < 0) return 0;
  struct stat sb;
  if (fstat(fd, &sb) != 0 || !S_ISREG(sb.st_mode))
    die(std::string(TOOL) + ": --bam needs a regular file, not a pipe: the BAM is mapped and read " + (SINGLE ? "once" : "twice"));
  if (!is_bgzf(fd, true, (uint64_t)sb.st_size)) die(std::string(TOOL) + ": --bam: '" + a.in1 + "' is not BGZF");
  const std::vector<uint64_t> keys = load_keys(text, a.k, TOOL);
  const std::vector<int> gpus = gpu_list();
  if (gpus.size() != 1)
    die(std::string(TOOL) + ": --bam finds, scans and pulls the records on the device, which needs one device (RUFUS_GPUS names "
        "more)");
  Outputs out;
  if (!out.open(a.chr, a.stub)) return 0;
  Devices dv;
  dv.open(gpus, keys, a.k, "filter --bam: device open, set built");
  const Mapped bam = map_regular(fd, true);
  if (!bam.ok) die(std::string(TOOL) + ": --bam: cannot map the input: " + strerror(errno));
  const size_t arena = env_arena("RFX_BAM_ARENA"), piece = env_piece((size_t)8 << 20);
  if constexpr (SINGLE) {
    BamSingleFilter route(
        dv.ctxs[0], dv.sets[0], a.min_q, a.thresh, a.exclude, [&](const char* p, size_t n) { out.out1.write(p, (std::streamsize)n); },
        arena, piece);
    if (a.region) route.set_region(a.region, a.in1);
    route.run(bam.p, bam.n);
    out.finish(route.chr_log(), "", "", route.counts());
  } else {
    BamPairFilter route(dv.ctxs[0], dv.sets[0], a.min_q, a.thresh, a.exclude, arena, piece);
    if (a.region) route.set_region(a.region, a.in1);
    route.run(bam.p, bam.n);
    out.finish(route.chr_log(), route.mate1(), route.mate2(), route.counts());
  }
  dv.close();
  return 0;
}

// `RUFUS.Filter --packed CACHE CHRFILE PreBuiltMutHash X.bam firstpassfile hashsize MinQ HashCountThreshold threads` with the
// BAM-kind cache `jellyfish count --bam CHR --keep-packed CACHE X.bam` left (rfx_bam_cache.hpp): what `--bam` writes, byte
// for byte, without a pass over the file -- the cache is scanned, and only the BGZF blocks that hold the hit names' records
// are read and inflated (rfx_ingest.hpp BamCachePull).  Replaces the two inflates of runRufus.sh:964-967's generator that
// `--bam` still does.  A cache that read_cache refuses, one made for another MinQ or other exclude flags than `--bam`'s
// 3328, an X.bam that is not a regular BGZF file of the recorded size, or a fetched record that is not the record the cache
// describes: one line on stderr and the two-pass `--bam` route in this process, with the same arguments.  One device.
// Paired only; samf::run_packed sends it here.
static int run_cached(const FilterArgs& a) {
  const std::vector<int> gpus = gpu_list();
  if (gpus.size() != 1)
    die("rufus_amd RUFUS.Filter: --packed with a BAM's cache scans and fetches on the device, which needs one device (RUFUS_GPUS "
        "names more)");
  auto two_pass = [&]() {
    fprintf(stderr, "rufus_amd RUFUS.Filter: %s is not a usable packed-read cache of %s for MinQ %d: reading the BAM twice\n", a.cache,
            a.in1, a.min_q);
    fputs(USAGE, stdout);
    return run(a);  // (--packed takes neither --bam-exclude nor --region: a holds --bam's defaults)
  };
  // the cache, mapped and checked
  rfxbamcache::Cache cache;
  const Mapped cm = map_regular(a.cache, false);
  if (!cm.ok || !rfxbamcache::read_cache(cm.p, cm.n, cache) || cache.h.min_q != a.min_q || cache.h.exclude_flags != 3328u) return two_pass();
  struct stat bs;
  if (stat(a.in1, &bs) != 0 || !S_ISREG(bs.st_mode) || (uint64_t)bs.st_size != cache.h.bam_bytes) return two_pass();
  std::string text;
  if (!read_hash_list(a.hashlist, text)) return 0;
  const std::vector<uint64_t> keys = load_keys(text, a.k, TOOL);
  const size_t arena = env_arena("RFX_BAM_ARENA"), piece = env_piece((size_t)8 << 20);
  Devices dv;
  dv.open(gpus, keys, a.k, "filter --packed: device open, set built");
  bool same = true;
  {
    // (the fetch arena is a quarter of RFX_BAM_ARENA, the size of BamIngest's runs: it holds the few blocks of the selection,
    // not a stretch of the file)
    BamCachePull route(dv.ctxs[0], dv.sets[0], a.thresh, arena / 4, piece);
    route.scan(cache);
    trace("filter --packed: cache scanned");
    if (route.hits()) {  // (no hit: the BAM is not opened)
      const int fd = ::open(a.in1, O_RDONLY);
      const Mapped bam = map_regular(fd, false);
      same = bam.ok && (uint64_t)bam.n == cache.h.bam_bytes && is_bgzf(fd, true, (uint64_t)bam.n);
      if (fd >= 0) ::close(fd);
      same = same && route.pull(cache, bam.p, bam.n);
      if (bam.p) munmap((void*)bam.p, bam.n);
    }
    if (same) {
      Outputs out;
      if (!out.open(a.chr, a.stub)) return 0;
      out.finish(route.chr_log(), route.mate1(), route.mate2(), route.counts());
    }
  }
  dv.close();
  return same ? 0 : two_pass();  // (a fetched record was not the cache's: nothing has been written)
}
}  // namespace bamf

// `RUFUS.Filter --packed CACHE CHRFILE PreBuiltMutHash SPOOL firstpassfile hashsize MinQ HashCountThreshold threads`
// (rfx_packed_cache.hpp): the subject's records were packed once, by `jellyfish count --sam ..
// --keep-packed CACHE`.  Here they are uploaded as they lie in CACHE and scanned; only the lines of the names with a hit
// are gathered from SPOOL (the stream's bytes: `--spool`, or the SAM file itself) and go through samf::run above.
// A CACHE that begins with rfx_bam_cache.hpp's magic is `jellyfish count --bam .. --keep-packed`'s: SPOOL is then the BAM
// file itself and the route is bamf::run_cached.  Paired only.
namespace samf {
static bool parse_packed(int argc, char** argv, FilterArgs& a) {
  printf("Call is --packed CACHE CHRFILE PreBuiltMutHash SPOOL firstpassfile hashsize MinQ HashCountThreshold threads\n");
  if (argc < 11) {
    printf("ERROR: expected 10 arguments\n");
    return false;
  }
  for (int i = 11; i < argc; ++i)
    if (strcmp(argv[i], "--region") == 0)
      die("rufus_amd RUFUS.Filter: --region does not go with --packed: the cache does not record a region (use --bam)");
  a.cache = argv[2];
  positional(a, argv + 3);
  return true;
}

static int run_packed(const FilterArgs& a) {
  {
    uint64_t magic = 0;
    const int cfd = ::open(a.cache, O_RDONLY);
    const bool bam_kind = cfd >= 0 && ::pread(cfd, &magic, 8, 0) == 8 && magic == rfxbamcache::FILE_MAGIC;
    if (cfd >= 0) ::close(cfd);
    if (bam_kind) return bamf::run_cached(a);
  }
  const char *cache_path = a.cache, *spool = a.in1;
  auto text_route = [&](const char* sam_path, const char* chr_to, bool has_caller) {  // the ordinary --sam route on `sam_path`
    FilterArgs b = a;
    b.in1 = sam_path;
    b.chr = chr_to;
    b.has_caller = has_caller;
    fputs(USAGE, stdout);
    return run(b);
  };
  std::vector<rfxcache::ChunkView> chunks;
  int cached_q = 0;
  const Mapped sm = map_regular(spool, false, true);
  if (!sm.ok) {
    printf("Error, MutFile could not be opened");
    return 0;
  }
  const Mapped cm = map_regular(cache_path, false, true);
  if (!cm.ok || !rfxcache::read_chunks(cm.p, cm.n, sm.n, cached_q, chunks) || cached_q != a.min_q) {
    // no cache, one its producer did not finish, a cache of another stream (length), or packed for another MinQ: the text decides
    fprintf(stderr, "rufus_amd RUFUS.Filter: %s is not a usable packed-read cache for MinQ %d: scanning the text\n", cache_path, a.min_q);
    return text_route(spool, a.chr, false);
  }
  std::string text;
  if (!read_hash_list(a.hashlist, text)) return 0;
  const std::vector<uint64_t> keys = load_keys(text, a.k, TOOL, false);  // (the text route below announces them)
  std::unordered_set<uint64_t> hit_names;
  uint64_t n_rec = 0, n_hit = 0, n_always = 0;
  {
    Devices dv;
    dv.open(gpu_list(), keys, a.k, "filter --packed: device open, set built");
    // chunk i goes to device i mod N; one thread per device uploads and scans (the arrays lie in the cache as the
    // upload wants them: no parsing, no packing)
    std::mutex mu;
    std::vector<std::thread> th;
    for (size_t d = 0; d < dv.size(); ++d)
      th.emplace_back([&, d] {
        std::vector<uint64_t> mask;
        std::vector<uint64_t> local;
        uint64_t rec = 0, hit = 0, always = 0;
        for (size_t i = d; i < chunks.size(); i += dv.size()) {
          const rfxcache::ChunkView& v = chunks[i];
          const uint32_t n = v.h->n;
          if (!n) continue;
          mask.assign(((size_t)n + 63) / 64, 0);
          dv.scan_block(d, v.codes, v.good, v.word_off, v.len, n, a.thresh, nullptr, mask.data());
          for (uint32_t r = 0; r < n; ++r) {
            const bool al = v.flags[r] & rfxcache::REC_ALWAYS;
            if (al || ((mask[r >> 6] >> (r & 63)) & 1)) {
              local.push_back(v.hash[r]);
              if (al) ++always; else ++hit;
            }
          }
          rec += n;
        }
        std::lock_guard<std::mutex> g(mu);
        hit_names.insert(local.begin(), local.end());
        n_rec += rec;
        n_hit += hit;
        n_always += always;
      });
    for (auto& t : th) t.join();
    dv.close();
  }
  trace("filter --packed: cache scanned");
  // every line whose name (hash) has a hit, in stream order
  std::string mini;
  uint64_t n_lines = 0;
  for (const rfxcache::ChunkView& v : chunks)
    for (uint32_t r = 0; r < v.h->n; ++r)
      if (hit_names.count(v.hash[r])) {
        const uint64_t at = v.h->stream_off + v.line_off[r];  // (inside the spool: read_chunks checked every line)
        // the line must be the record the chunk was made from: same QNAME (a cache left over from another stream of
        // the same length would otherwise hand the text route the wrong lines without anybody noticing)
        const char* ln = sm.p + at;
        const char* tab = (const char*)memchr(ln, '\t', v.line_len[r]);
        if (!tab || rfxsam::name_hash(ln, (size_t)(tab - ln)) != v.hash[r]) {
          fprintf(stderr, "rufus_amd RUFUS.Filter: %s does not describe %s (a line is not the record it was packed from): scanning the text\n",
                  cache_path, spool);
          return text_route(spool, a.chr, false);
        }
        mini.append(ln, v.line_len[r]);
        mini.push_back('\n');
        ++n_lines;
      }
  printf("\npacked cache: %llu records scanned, %llu hit, %llu left to the text route outright; %llu lines gathered\n",
         (unsigned long long)n_rec, (unsigned long long)n_hit, (unsigned long long)n_always, (unsigned long long)n_lines);
  // the chromosome log of the WHOLE stream (src/PassThroughSamCheck.stranded.cpp: "notachr", then every run of RNAME)
  {
    FILE* chr = fopen(a.chr, "w");
    if (!chr) {
      printf("ERROR, Output file could not be opened -%s\n", a.chr);
      return 0;
    }
    std::string current = "notachr";
    for (const rfxcache::ChunkView& v : chunks) {
      const char *p = v.runs, *e = v.runs + v.h->runs_bytes;
      while (p < e) {
        const char* nl = (const char*)memchr(p, '\n', (size_t)(e - p));
        if (!nl) nl = e;
        if (current.size() != (size_t)(nl - p) || memcmp(current.data(), p, current.size()) != 0) {
          fprintf(chr, "%s\n", current.c_str());
          current.assign(p, (size_t)(nl - p));
        }
        p = nl + 1;
      }
    }
    fprintf(chr, "%s\n", current.c_str());
    fclose(chr);
  }
  // the gathered lines through the text route (a file the route can map; its own chromosome log is not the stream's)
  const char* tmpdir = access("/dev/shm", W_OK) == 0 ? "/dev/shm" : "/tmp";
  std::string tmp = std::string(tmpdir) + "/rfx_packed_XXXXXX";
  const int tfd = mkstemp(&tmp[0]);
  if (tfd < 0) die("rufus_amd RUFUS.Filter --packed: cannot create a temporary file");
  for (size_t at = 0; at < mini.size();) {
    const ssize_t w = ::write(tfd, mini.data() + at, mini.size() - at);
    if (w < 0 && errno == EINTR) continue;
    if (w <= 0) die("rufus_amd RUFUS.Filter --packed: write error on the temporary file");
    at += (size_t)w;
  }
  ::close(tfd);
  const int rc = text_route(tmp.c_str(), "/dev/null", true);
  ::unlink(tmp.c_str());
  return rc;
}
}  // namespace samf

// ---- RUFUS.Filter HashList Mate1.fq Mate2.fq STUB ... / RUFUS.Filter.single HashList FQ|stdin STUB ...: FASTQ text --------
// Pipeline (the device scans ~1000x faster than one core parses, so the host side is what counts):
//   one reader per mate stream cuts it into pieces of PIECE_RECS records (4 lines each, counted blindly like the
//   reference's getline x 4); the two pipes are always being drained, so a writer in lock step
//   (PassThroughSamCheck.stranded, runRufus.sh:966) never blocks on the one while we wait on the other;
//   workers take piece i of both streams, find the lines, pack bases + quality mask of both mates
//   (rfx_pack_spans), run the scan (k_filter; device calls are serialised, they take microseconds) and format
//   the pulled records;
//   the main thread writes the formatted pieces in input order.
// The device is opened (0.1 - 0.25 s of runtime start-up) and the set built beside the readers and the workers' first
// pieces: a worker needs them when its first piece is packed (RFX_SYNC_OPEN=1: before anything else, as it used to be).
// A reader or a worker that has to refuse the input just calls die(): while the Opener lives, die() waits for the opener
// thread before it exits (rfx_cli.hpp).
namespace textf {
static bool parse(int argc, char** argv, FilterArgs& a) {
  const int need = SINGLE ? 8 : 9;
  fputs(SINGLE ? "Call is PreBuiltMutHash Mutant.fq|stdin firstpassfile hashsize MinQ HashCountThreshold threads\n"
               : "Call is PreBuiltMutHash Mutant.Mate1.fq Mutant.Mate2.fq firstpassfile hashsize MinQ HashCountThreshold threads \n",
        stdout);
  if (argc < need) {
    printf("ERROR: expected %d arguments\n", need - 1);
    return false;
  }
  int i = 1;
  a.hashlist = argv[i++];
  a.in1 = argv[i++];
  if (!SINGLE) a.in2 = argv[i++];
  a.stub = argv[i++];
  a.k = atoi(argv[i++]);
  a.min_q = atoi(argv[i++]);
  a.thresh = atoi(argv[i++]);
  a.threads = atoi(argv[i]);
  return true;
}

static const size_t PIECE_RECS = 1u << 16;
// A piece: PIECE_RECS records (the last one of a stream: fewer) = 4 * recs lines of text, each ending in '\n'.
// Its bytes are the piece's own buffer (filled by read()) or lie in the mapping of a regular input file.
struct Piece {
  const char* data = nullptr;
  size_t size = 0, recs = 0;
  std::unique_ptr<char[]> own;
  size_t cap = 0;
};
struct Stream {
  int fd = -1;
  std::mutex mu;
  std::condition_variable cv;
  std::deque<Piece*> q;
  bool done = false;
  bool abort = false;         // mate 1 ended: nobody takes this stream's pieces any more
  const char* map = nullptr;  // regular file: mapped
  size_t map_size = 0;
};
struct Result { std::string out1, out2; unsigned long long recs = 0, found = 0; bool ready = false; };

static int run(const FilterArgs& a) {
  const int min_q = a.min_q, thresh = a.thresh;
  const int n_streams = SINGLE ? 1 : 2;
  std::string text;
  if (!read_hash_list(a.hashlist, text)) return 0;
  Stream st[2];
  if ((st[0].fd = open_input(a.in1, 2)) < 0) return 0;
  if (!SINGLE && (st[1].fd = open_input(a.in2, 0)) < 0) return 0;
  Outputs out;
  if (!out.open(nullptr, a.stub)) return 0;
  const std::vector<uint64_t> keys = load_keys(text, a.k, "rufus_amd RUFUS.Filter");
  trace("filter: hash list parsed");
  if constexpr (!SINGLE) {  // two bgzip'd mate files: the device inflates them (namespace bgzff); one of the two is a mistake
    bool z[2];
    for (int m = 0; m < 2; ++m) {
      struct stat sb;
      const bool regular = st[m].fd != 0 && fstat(st[m].fd, &sb) == 0 && S_ISREG(sb.st_mode);
      z[m] = is_bgzf(st[m].fd, regular, regular ? (uint64_t)sb.st_size : 0);
    }
    if (z[0] != z[1])
      die(std::string("rufus_amd RUFUS.Filter: ") + (z[0] ? a.in1 : a.in2) + " is BGZF and " + (z[0] ? a.in2 : a.in1) +
          " is not: give both mates compressed or both as text");
    if (z[0]) return bgzff::run(a, st[0].fd, st[1].fd, keys, out);
  }
  // RUFUS_GPUS: the pieces are dealt to the devices by worker thread (the filter shards by read block)
  const std::vector<int> gpus = gpu_list();
  const size_t n_gpu = gpus.size();
  Devices dv;  // (the opener's until Opener::wait() has returned)
  Opener opener([&] { dv.open(gpus, keys, a.k, "filter: device open, set built"); });
  if (getenv("RFX_SYNC_OPEN")) Opener::wait();

  for (int i = 0; i < n_streams; ++i) {
    const Mapped m = getenv("RFX_FILTER_NO_MMAP") ? Mapped() : map_regular(st[i].fd, true);
    st[i].map = m.p;
    st[i].map_size = m.n;
#ifdef F_SETPIPE_SZ
    if (!m.ok) (void)fcntl(st[i].fd, F_SETPIPE_SZ, 1 << 20);  // a pipe: fewer, larger reads (ignored on anything else)
#endif
  }
  const skip_lines_fn skip_lines = pick_skip_lines();
  const index_lines_fn index_lines = pick_index_lines();
  const size_t MAX_AHEAD = 48;  // pieces a reader may be ahead of the workers (~1 GB of text per stream)
  auto new_piece = [](size_t cap) {
    Piece* p = new Piece();
    p->own.reset(new char[cap]);  // (not value-initialised: nothing is written that read() will not overwrite)
    p->cap = cap;
    p->data = p->own.get();
    return p;
  };
  auto grow = [](Piece* p, size_t cap) {
    std::unique_ptr<char[]> nb(new char[cap]);
    memcpy(nb.get(), p->data, p->size);
    p->own = std::move(nb);
    p->cap = cap;
    p->data = p->own.get();
  };
  auto reader = [&](Stream& S) {
    auto push = [&](Piece* pc) {
      std::unique_lock<std::mutex> g(S.mu);
      S.cv.wait(g, [&] { return S.q.size() < MAX_AHEAD || S.abort; });
      if (S.abort) {  // (the reference stops at the end of file 1: what mate 2 still holds is read and dropped)
        delete pc;
        return;
      }
      S.q.push_back(pc);
      S.cv.notify_all();
    };
    // the end of a stream, std::getline semantics: a final unterminated line still counts, and the missing lines
    // of an incomplete last record read as empty
    auto finish_tail = [&](Piece* cur, size_t lines) {
      if (cur->size) {
        if (cur->cap < cur->size + 8) grow(cur, cur->size + 8);
        char* d = cur->own.get();
        if (d[cur->size - 1] != '\n') {
          d[cur->size++] = '\n';
          ++lines;
        }
        cur->recs = (lines + 3) / 4;
        while (lines < 4 * cur->recs) {
          d[cur->size++] = '\n';
          ++lines;
        }
      }
      std::lock_guard<std::mutex> g(S.mu);
      if (cur->recs) S.q.push_back(cur);
      else delete cur;
      S.done = true;
      S.cv.notify_all();
    };
    if (S.map) {  // cut the mapping in place: only the last piece is copied (it may need lines added)
      const char *p = S.map, *e = S.map + S.map_size;
      for (;;) {
        size_t got;
        const char* cut = skip_lines(p, e, 4 * PIECE_RECS, got);
        if (got == 4 * PIECE_RECS) {
          Piece* pc = new Piece();
          pc->data = p;
          pc->size = (size_t)(cut - p);
          pc->recs = PIECE_RECS;
          push(pc);
          p = cut;
          continue;
        }
        Piece* last = new_piece((size_t)(e - p) + 8);
        memcpy(last->own.get(), p, (size_t)(e - p));
        last->size = (size_t)(e - p);
        finish_tail(last, got);
        return;
      }
    }
    const size_t CAP0 = PIECE_RECS * 360, RD = 1u << 20;
    Piece* cur = new_piece(CAP0);
    size_t lines = 0, scanned = 0;
    for (;;) {
      if (cur->cap - cur->size < RD) grow(cur, cur->cap + cur->cap / 2 + RD);
      const ssize_t n = ::read(S.fd, cur->own.get() + cur->size, RD);
      if (n < 0 && errno == EINTR) continue;
      if (n < 0) die(std::string("read error on input: ") + strerror(errno));
      if (n == 0) break;
      cur->size += (size_t)n;
      while (scanned < cur->size) {
        size_t got;
        const char* stop = skip_lines(cur->data + scanned, cur->data + cur->size, 4 * PIECE_RECS - lines, got);
        lines += got;
        scanned = (size_t)(stop - cur->data);
        if (lines < 4 * PIECE_RECS) break;  // (stop == end of what has been read)
        Piece* nx = new_piece(CAP0);
        nx->size = cur->size - scanned;
        memcpy(nx->own.get(), cur->data + scanned, nx->size);
        cur->size = scanned;
        cur->recs = PIECE_RECS;
        push(cur);
        cur = nx;
        lines = 0;
        scanned = 0;
      }
    }
    finish_tail(cur, lines);
  };
  std::thread readers[2];
  for (int i = 0; i < n_streams; ++i) readers[i] = std::thread(reader, std::ref(st[i]));

  std::mutex res_mu, take_mu;
  std::condition_variable res_cv;
  std::map<uint64_t, Result> results;
  uint64_t next_seq = 0;
  bool input_done = false;
  auto take = [&](Piece*& p1, Piece*& p2, uint64_t& seq) -> bool {  // piece `seq` of both streams, in order
    std::lock_guard<std::mutex> tg(take_mu);
    p1 = p2 = nullptr;
    {
      std::unique_lock<std::mutex> g(st[0].mu);
      st[0].cv.wait(g, [&] { return !st[0].q.empty() || st[0].done; });
      if (st[0].q.empty()) {
        {
          std::lock_guard<std::mutex> rg(res_mu);
          input_done = true;
          res_cv.notify_all();
        }
        if (n_streams == 2) {  // a mate-2 reader waiting for room must not wait for ever
          std::lock_guard<std::mutex> g2(st[1].mu);
          st[1].abort = true;
          st[1].cv.notify_all();
        }
        return false;
      }
      p1 = st[0].q.front();
      st[0].q.pop_front();
      st[0].cv.notify_all();
    }
    if (n_streams == 2) {
      std::unique_lock<std::mutex> g(st[1].mu);
      st[1].cv.wait(g, [&] { return !st[1].q.empty() || st[1].done; });
      if (!st[1].q.empty()) {
        p2 = st[1].q.front();
        st[1].q.pop_front();
        st[1].cv.notify_all();
      } else {
        p2 = new Piece();  // mate 2 ran out: its records read as empty (lock step: one per record of mate 1)
      }
    }
    seq = next_seq++;
    return true;
  };
  auto worker = [&](unsigned me) {
    const size_t dev = (size_t)me % n_gpu;
    bool up = false;  // the opener is done: known by the first upload at the latest (Opener::wait() before it)
    std::vector<uint64_t> ls[2], ss[2], qs[2], mask;  // line starts, sequence / quality starts
    std::vector<uint32_t> sl[2], hits;
    std::vector<char> fix;  // private copies of quality strings that are shorter than their read
    Staging stage;
    for (;;) {
      Piece *pc[2];
      uint64_t seq;
      if (!take(pc[0], pc[1], seq)) return;
      const size_t n = pc[0]->recs;
      for (int m = 0; m < n_streams; ++m) {
        const char* t = pc[m]->data;
        const size_t tsize = pc[m]->size;
        // (one line start more than the records need: a mate-2 piece may hold more records than mate 1's -- the extra
        // ones are never looked at, as the reference stops at the end of file 1 -- and the last record's quality line
        // must end where line 4n starts, not at the end of the piece)
        ls[m].resize(4 * n + 2);
        const size_t found_lines = index_lines(t, t + tsize, ls[m].data(), 4 * n + 1);
        for (size_t li = found_lines; li <= 4 * n; ++li) ls[m][li] = tsize;  // (mate 2 ran out: empty lines)
        ss[m].resize(n);
        qs[m].resize(n);
        sl[m].resize(n);
        for (size_t i = 0; i < n; ++i) {
          auto len_of = [&](size_t line) {
            const uint64_t a0 = ls[m][line], a1 = ls[m][line + 1];
            return a1 > a0 ? (uint32_t)(a1 - a0 - 1) : 0u;  // without the '\n'
          };
          ss[m][i] = ls[m][4 * i + 1];
          sl[m][i] = len_of(4 * i + 1);
          qs[m][i] = ls[m][4 * i + 3];
          if (m == 0 && sl[m][i] == 0)
            die("rufus_amd RUFUS.Filter: empty sequence line (undefined behaviour in the reference) -- rejected");
        }
      }
      // pack: reads of mate 1, then of mate 2, into one block
      const size_t nr = n * (size_t)n_streams;
      uint64_t words = 0;
      for (int m = 0; m < n_streams; ++m)
        for (size_t i = 0; i < n; ++i) words += (sl[m][i] + 31) / 32;
      if (!stage.need(words, nr, up)) die(NO_STAGING);
      uint32_t w0 = 0;
      for (int m = 0; m < n_streams; ++m) {
        const char* t = pc[m]->data;
        uint32_t *woff = stage.woff + m * n, *lens = stage.lens + m * n;
        woff[0] = w0;
        // Runs of ordinary reads are packed in place.  A quality line shorter than its read would make the packer
        // read the next line's bytes: such a read is packed on its own from a private copy of its sequence and
        // quality string, the latter padded with '\0' (= bad, what the reference's missing chars are).
        size_t at = 0;
        while (at < n) {
          size_t run = at;
          auto qlen = [&](size_t i) {
            const uint64_t q0 = ls[m][4 * i + 3], q1 = ls[m][4 * i + 4];
            return q1 > q0 ? (uint32_t)(q1 - q0 - 1) : 0u;
          };
          while (run < n && qlen(run) >= sl[m][run]) ++run;
          if (run > at &&
              rfx_pack_spans(t, ss[m].data() + at, sl[m].data() + at, qs[m].data() + at, (uint32_t)(run - at), min_q,
                             RFX_PACK_FILTER, stage.codes, nullptr, stage.good, woff + at, lens + at) != RFX_OK)
            die("rufus_amd: pack failed");
          if (run < n) {
            const uint32_t L = sl[m][run], ql = qlen(run);
            fix.assign((size_t)2 * L, '\0');
            memcpy(fix.data(), t + ss[m][run], L);
            memcpy(fix.data() + L, t + qs[m][run], ql);
            const uint64_t s0 = 0, q0 = L;
            if (rfx_pack_spans(fix.data(), &s0, &L, &q0, 1, min_q, RFX_PACK_FILTER, stage.codes, nullptr, stage.good, woff + run,
                               lens + run) != RFX_OK)
              die("rufus_amd: pack failed");
            ++run;
          }
          at = run;
        }
        w0 = woff[n];
      }
      mask.assign((nr + 63) / 64, 0);
      if (SINGLE) hits.assign(nr, 0);
      if (!up) {
        Opener::wait();
        up = true;
        stage.lock();
      }
      dv.scan_block(dev, stage.codes, stage.good, stage.woff, stage.lens, (uint32_t)nr, thresh, SINGLE ? hits.data() : nullptr,
                    mask.data());
      Result res;
      res.recs = n;
      auto bit = [&](size_t r) { return (mask[r >> 6] >> (r & 63)) & 1; };
      auto put = [&](std::string& o, int m, size_t i, const char* suffix) {
        const char* t = pc[m]->data;
        for (int j = 0; j < 4; ++j) {
          const uint64_t a0 = ls[m][4 * i + j], a1 = ls[m][4 * i + j + 1];
          const size_t len = a1 > a0 ? (size_t)(a1 - a0 - 1) : 0;
          o.append(t + a0, len);
          if (j == 0 && suffix) o.append(suffix);
          o.push_back('\n');
        }
      };
      for (size_t i = 0; i < n; ++i) {
        if (SINGLE) {
          if (bit(i)) {
            const std::string suffix = ":MH" + std::to_string(hits[i]);
            put(res.out1, 0, i, suffix.c_str());
            ++res.found;
          }
        } else if (bit(i) | bit(n + i)) {  // == the reference's "mate 2 only if mate 1 failed" (:237-277)
          put(res.out1, 0, i, nullptr);
          put(res.out2, 1, i, nullptr);
          ++res.found;
        }
      }
      for (int m = 0; m < n_streams; ++m) {
        if (!pc[m]->own && st[m].map) drop_mapped(pc[m]->data, pc[m]->data + pc[m]->size);  // a range of the file's mapping
        delete pc[m];
      }
      res.ready = true;
      std::lock_guard<std::mutex> g(res_mu);
      results[seq] = std::move(res);
      res_cv.notify_all();
    }
  };
  unsigned nthreads = (unsigned)std::max(1, a.threads);
  nthreads = std::min(nthreads, rfx_host_cpus());
  if (const char* ev = getenv("RFX_HOST_THREADS")) nthreads = (unsigned)std::max(1, atoi(ev));
  nthreads = std::max(nthreads, (unsigned)n_gpu);
  std::vector<std::thread> workers;
  for (unsigned t = 0; t < nthreads; ++t) workers.emplace_back(worker, t);
  unsigned long long found = 0, total = 0;
  for (uint64_t want = 0;; ++want) {
    Result res;
    {
      std::unique_lock<std::mutex> g(res_mu);
      res_cv.wait(g, [&] { return results.count(want) || (input_done && want >= next_seq); });
      if (!results.count(want)) break;
      res = std::move(results[want]);
      results.erase(want);
    }
    out.out1.write(res.out1.data(), (std::streamsize)res.out1.size());
    out.out2.write(res.out2.data(), (std::streamsize)res.out2.size());
    total += res.recs;
    found += res.found;
    printf("Read in %llu lines: Found %llu \r", total * 4, found);
  }
  trace("filter: all pieces written");
  opener.join();
  out.finish({}, "", "", "");
  for (auto& w : workers) w.join();
  for (int i = 0; i < n_streams; ++i) readers[i].join();
  dv.close();
  trace("filter: closed");
  return 0;
}
}  // namespace textf

int main(int argc, char** argv) {
  const char* flag = argc > 1 ? argv[1] : "";
  FilterArgs a;
  if (strcmp(flag, "--sam") == 0) return samf::parse(argc, argv, a) ? samf::run(a) : 0;
  if (strcmp(flag, "--bam") == 0) return bamf::parse(argc, argv, a) ? bamf::run(a) : 0;
  if (strcmp(flag, "--packed") == 0) {
    if constexpr (SINGLE)
      die("rufus_amd RUFUS.Filter.single: --packed is for paired subjects only (RUFUS.Filter --packed): use --bam or --sam");
    else
      return samf::parse_packed(argc, argv, a) ? samf::run_packed(a) : 0;
  }
  return textf::parse(argc, argv, a) ? textf::run(a) : 0;
}
