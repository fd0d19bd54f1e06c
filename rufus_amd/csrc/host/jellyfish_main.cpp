// Drop-in `jellyfish` for the sub-commands RUFUS runs on its hot path, same argv and file formats:
//   count  --disk -m K -L L -s SIZE -t T -o OUT -C IN...      scripts/RunJellyForRUFUS.sh:29
//   histo  -f -o OUT DB                                        scripts/RunJellyForRUFUS.sh:37
//   query  -s FASTA DB                                         scripts/CheckJellyHashList.sh:12
//   dump   -c DB                                               scripts/Overlap.shorter.sh:247
//   merge  F1 F2 ...   (RUFUS's MODIFIED merge: prints the k-mers unique to one input, count >= 5)
//                                                              runRufus.sh:925, jf/jellyfish/merge_files.cc:69-155
// Install it at both $RDIR/bin/externals/jellyfish/src/jellyfish_project/bin/jellyfish and
// $RDIR/bin/externals/modified_jellyfish/src/modified_jellyfish_project/bin/jellyfish.
// Host code only parses text and moves bytes; counting, sorting, set difference and lookups run in
// the HIP kernels behind include/rufus_hip.h.  No CPU fallback.
#include <getopt.h>

#include "rfx_ingest.hpp"

using namespace rfxcli;

static double now() {  // seconds on the steady clock
  return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// ---------------------------------------------------------------------------------------------
// `jellyfish count`: count_main, at the end of this section, reads as its steps.
struct CountArgs {
  int k = 0, threads = 1, out_counter_len = 4, lsize = 1;  // lsize: -s SIZE as a power of two, rounded up
  uint64_t lower = 0, upper = std::numeric_limits<uint64_t>::max();
  bool canonical = false;
  const char* out = "mer_counts.jf";
  const char* timing = nullptr;
  // --sam CHR_FILE (not in jellyfish): the input is SAM text and this process does what
  // `PassThroughSamCheck CHR_FILE | jellyfish count` does (scripts/RunJellyForRUFUS.sh:28-29) -- the sequence of
  // every record counted, the chromosome log written -- without the FASTQ text in between: SURVEY 8 row N1.
  const char* sam_chr = nullptr;
  // --spool FILE (not in jellyfish): the bytes of a PIPE input are also written to FILE, so that the
  // stage that reads the same stream next (RUFUS.Filter on the subject, runRufus.sh:966) reads FILE instead of
  // running the subject's generator -- `samtools view` of a BAM -- a second time (`RUFUS.Filter --sam CHR HashList FILE ...`).
  const char* spool_path = nullptr;
  // --keep-packed FILE [--keep-minq Q] (not in jellyfish; SURVEY 8 row N2, with --sam): the parser threads also leave the
  // records as RUFUS.Filter would see them -- printed orientation, packed for MinQ Q (default 15), name hash, place in
  // the stream -- in FILE (rfx_packed_cache.hpp; put it in /dev/shm): `RUFUS.Filter --packed FILE CHR HashList SPOOL ...`
  // scans that instead of parsing the stream a second time.
  // With --bam (ONE input): the BAM-kind cache of rfx_bam_cache.hpp -- per arena the filter's view of the kept records as
  // the device packs it, their name hashes and their addresses in the inflated stream, and an index of the file's BGZF
  // blocks -- so that `RUFUS.Filter --packed FILE CHR HashList X.bam ...` inflates only the blocks of the hit names'
  // records instead of the whole file twice (runRufus.sh:964-967 after scripts/RunJellyForRUFUS.sh:28-29).
  const char* keep_path = nullptr;
  int keep_minq = 15;
  // --bam CHR_FILE [--bam-exclude N] (not in jellyfish): the input is a BAM file and this process does what
  // `samtools view -F N X.bam | PassThroughSamCheck CHR_FILE | jellyfish count` does (runRufus.sh:599,
  // scripts/RunJellyForRUFUS.sh:28-29; N defaults to 3328) -- BGZF inflated, the records found and their sequences packed
  // on the device (rfx_ingest.hpp BamIngest; csrc/rfx_bam.hip), the chromosome log written.  Goes with --keep-packed
  // (above), not with --sam or --spool.
  const char* bam_chr = nullptr;
  uint32_t bam_exclude = 3328;
  // --region REG (with --bam, ONE input; not in jellyfish): `samtools view -F N X.bam REG`, what runRufus.sh -R puts into the
  // generator -- only the records that overlap CHR[:BEG[-END]] are counted and logged; X.bam.bai / X.bai, when there, limits
  // what is inflated (rfx_bai.hpp, BamIngest::set_region).  Not with --keep-packed: the cache does not record a region.
  const char* bam_region = nullptr;
  std::vector<const char*> inputs;
  bool plain() const { return !sam_chr && !spool_path && !keep_path; }  // no route-limiting option but --bam
};
static const char* const BAM_ALONE = "rufus_amd jellyfish count: --bam finds and packs the records on the device, which needs one "
                                     "device and none of --sam, --spool, --keep-packed";

// The option table and every refusal that needs neither an input nor a device.
static void parse_count(int argc, char** argv, CountArgs& a) {
  uint64_t size = 0;
  bool size_given = false;
  enum { OPT_DISK = 1000, OPT_OCL, OPT_TIMING, OPT_TEXT, OPT_SAM, OPT_SPOOL, OPT_KEEP, OPT_KEEPQ, OPT_BAM, OPT_BAMX, OPT_REGION };
  static option lo[] = {{"mer-len", 1, 0, 'm'},      {"size", 1, 0, 's'},        {"threads", 1, 0, 't'},
                        {"output", 1, 0, 'o'},       {"counter-len", 1, 0, 'c'}, {"out-counter-len", 1, 0, OPT_OCL},
                        {"canonical", 0, 0, 'C'},    {"disk", 0, 0, OPT_DISK},   {"lower-count", 1, 0, 'L'},
                        {"upper-count", 1, 0, 'U'},  {"timing", 1, 0, OPT_TIMING}, {"text", 0, 0, OPT_TEXT}, {"sam", 1, 0, OPT_SAM},
                        {"spool", 1, 0, OPT_SPOOL},  {"keep-packed", 1, 0, OPT_KEEP}, {"keep-minq", 1, 0, OPT_KEEPQ},
                        {"bam", 1, 0, OPT_BAM},      {"bam-exclude", 1, 0, OPT_BAMX}, {"region", 1, 0, OPT_REGION},
                        {"reprobes", 1, 0, 'p'},     {0, 0, 0, 0}};
  optind = 1;
  int ch;
  while ((ch = getopt_long(argc, argv, "m:s:t:o:c:CL:U:p:", lo, nullptr)) != -1) {
    switch (ch) {
      case 'm': a.k = atoi(optarg); break;
      case 's': if (!parse_si(optarg, size)) die(std::string("Invalid size '") + optarg + "'"); size_given = true; break;
      case 't': a.threads = atoi(optarg); break;
      case 'o': a.out = optarg; break;
      case 'c': break;  // in-memory counter width of the reference table: no meaning here
      case 'p': break;
      case 'C': a.canonical = true; break;
      case 'L': if (!parse_si(optarg, a.lower)) die("Invalid lower count"); break;
      case 'U': if (!parse_si(optarg, a.upper)) die("Invalid upper count"); break;
      case OPT_DISK: break;  // table growth / merging is internal
      case OPT_OCL: a.out_counter_len = atoi(optarg); break;
      case OPT_TIMING: a.timing = optarg; break;
      case OPT_SAM: a.sam_chr = optarg; break;
      case OPT_SPOOL: a.spool_path = optarg; break;
      case OPT_KEEP: a.keep_path = optarg; break;
      case OPT_KEEPQ: a.keep_minq = atoi(optarg); break;
      case OPT_BAM: a.bam_chr = optarg; break;
      case OPT_BAMX: a.bam_exclude = (uint32_t)strtoul(optarg, nullptr, 0); break;
      case OPT_REGION:
        if (a.bam_region) die("rufus_amd jellyfish count: --region given twice: one region per run");
        a.bam_region = optarg;
        break;
      case OPT_TEXT: die("rufus_amd jellyfish: --text output is not on the RUFUS path");
      default: die("Usage: jellyfish count -m K -s SIZE [-C] [-L n] [-U n] [-t T] [-o OUT] [--disk] file...");
    }
  }
  a.inputs.assign(argv + optind, argv + argc);
  if (a.k < 1 || !size_given) die("Missing required switch: -m, --mer-len and -s, --size");
  if (a.inputs.empty()) die("Missing sequence file");
  if (a.bam_chr && (a.sam_chr || a.spool_path)) die(BAM_ALONE);
  if (a.bam_region && !a.bam_chr) die("rufus_amd jellyfish count: --region goes with --bam CHR_FILE: only a BAM's records carry a position");
  if (a.bam_region && a.keep_path)
    die("rufus_amd jellyfish count: --region does not go with --keep-packed: the cache does not record a region");
  if (a.bam_region && a.inputs.size() != 1) die("rufus_amd jellyfish count: --region goes with ONE input: the region names one file's references");
  while ((1ull << a.lsize) < size) ++a.lsize;
}

// Inputs: regular files are mapped (their size is known), pipes are streamed.  When the input is a pipe (its size is unknown:
// RUFUS feeds 30x genomes through FIFOs, scripts/RunJellyForRUFUS.sh:23-31) or a big file, the packed read blocks stay in HBM
// and are counted in minimizer-shard passes at finish (rfx_count_set_passes: bounded HBM, the analogue of --disk).
struct Input { std::string path; int fd; bool regular; size_t size; };

// The devices of a count: contexts, tables, the peer group and the read blocks that stay in HBM for the shard passes.
// open() runs on the opener thread (rfx_cli.hpp Opener) while the main thread starts the output's page allocation and the
// parser threads: the staging blocks are plain memory until their first upload (rfx_host_alloc_lazy / rfx_host_pin), so
// parsing needs no device (round 6: ~0.3 s of a 1.3 s count of 64 M reads).  What touches a ctx or a table passes
// Opener::wait() first.  RUFUS_GPUS: one sample over several devices (rfx_count_set_peers).
struct CountDevices {
  const std::vector<int> gpus;
  bool defer = false;  // count in shard passes at finish: survey() says, before open()
  std::vector<rfx_ctx*> ctxs;
  std::vector<rfx_table*> tabs;
  rfx_peers* peers = nullptr;
  std::vector<std::vector<rfx_reads*>> resident;
  // A sample counted in shard passes at finish needs ~3 bytes of device memory per byte of packed reads beside them
  // (records of a pass, survivors): it is mapped while the input is still parsed, a few GiB per uploaded block -- in a fresh
  // process mapping 130 GB took 0.6 s of the time between "input parsed" and "finished on the device".
  std::vector<uint64_t> reserved;
  std::vector<std::mutex> mu;  // (one upload at a time per device: the table of a device is not re-entrant)
  // Several devices: block b of packed reads goes to device b mod N; the owners of the minimizer bins pull their record runs at
  // finish (rfx_count_set_peers).  RFX_PEERS_REPLICATE=1: round 3's scheme, every block to EVERY device, one thread per device.
  const bool replicate = getenv("RFX_PEERS_REPLICATE") != nullptr;
  std::atomic<uint64_t> next_block{0};

  explicit CountDevices(const std::vector<int>& g) : gpus(g), resident(g.size()), reserved(g.size(), 0), mu(g.size()) {}
  int n() const { return (int)gpus.size(); }
  void open(const CountArgs& a) {
    ctxs = open_ctxs(gpus);
    peers = n() > 1 ? rfx_peers_create(n()) : nullptr;
    for (int g = 0; g < n(); ++g) {
      rfx_table* tb = rfx_count_begin(ctxs[(size_t)g], a.k, a.canonical, a.lsize, 0, 0, 0);
      if (!tb) die(std::string("rufus_amd: ") + rfx_last_error());
      tabs.push_back(tb);
    }
    trace("count: device open, table made");
    for (int g = 0; g < n(); ++g) {
      if (defer && rfx_count_set_passes(tabs[(size_t)g], 0) != RFX_OK) die(std::string("rufus_amd: ") + rfx_last_error());
      if (peers && rfx_count_set_peers(tabs[(size_t)g], peers, g) != RFX_OK) die(std::string("rufus_amd: ") + rfx_last_error());
    }
  }
  // one uploaded block into device g's table: counted and freed, or kept for the passes with room reserved beside it
  void sink_to(int g, rfx_reads* r) {
    Opener::wait();
    if (!r) die(std::string("rufus_amd: upload failed: ") + rfx_last_error());
    const int rc = rfx_count_add(tabs[(size_t)g], r);
    if (rc) die(std::string("rufus_amd: count failed: ") + rfx_strerror(rc) + " " + rfx_last_error());
    if (!defer) return rfx_reads_free(r);
    resident[(size_t)g].push_back(r);
    uint64_t used = 0, peak = 0, mapped = 0;
    if (getenv("RFX_NO_RESERVE") || rfx_mem_stats(ctxs[(size_t)g], &used, &peak, &mapped) != RFX_OK) return;
    const uint64_t want = std::min<uint64_t>(used * 4, 200ull << 30);
    if (want > reserved[(size_t)g] + (4ull << 30))  // (in steps of >= 4 GiB; a refusal is no error: mapped when needed)
      reserved[(size_t)g] = rfx_mem_reserve(ctxs[(size_t)g], want) == RFX_OK ? want : ~0ull >> 1;
  }
  // a block of the host parsers, uploaded by `up`: to the one device, to the next in turn, or to every one
  void to_all(const std::function<rfx_reads*(rfx_ctx*)>& up) {
    Opener::wait();
    if (n() == 1) {
      sink_to(0, up(ctxs[0]));
    } else if (!replicate) {
      const int g = (int)(next_block.fetch_add(1) % (uint64_t)n());
      std::lock_guard<std::mutex> lk(mu[(size_t)g]);
      sink_to(g, up(ctxs[(size_t)g]));
    } else {
      std::vector<std::thread> th;
      for (int g = 0; g < n(); ++g) th.emplace_back([&, g] { sink_to(g, up(ctxs[(size_t)g])); });
      for (auto& t : th) t.join();
    }
  }
  // one record set per device (several: the finishes meet at the survivor exchange, one thread each); `hist`: null, or zeroed bins
  std::vector<rfx_records*> finish(uint64_t lower, uint64_t upper, uint64_t* hist) {
    std::vector<rfx_records*> recs((size_t)n(), nullptr);
    if (n() == 1) {
      recs[0] = rfx_count_finish(tabs[0], lower, upper, hist);
    } else {
      std::vector<std::vector<uint64_t>> hs((size_t)n(), std::vector<uint64_t>(hist ? RFX_HISTO_BINS : 0));
      std::vector<std::thread> th;
      for (int g = 0; g < n(); ++g)
        th.emplace_back([&, g] { recs[(size_t)g] = rfx_count_finish(tabs[(size_t)g], lower, upper, hist ? hs[(size_t)g].data() : nullptr); });
      for (auto& t : th) t.join();
      for (int i = 0; hist && i < RFX_HISTO_BINS; ++i)
        for (int g = 0; g < n(); ++g) hist[i] += hs[(size_t)g][(size_t)i];
    }
    for (rfx_records* r : recs)
      if (!r) die(std::string("rufus_amd: finish failed: ") + rfx_last_error());
    trace("count: finished on the device");
    for (auto& v : resident)
      for (rfx_reads* r : v) rfx_reads_free(r);
    return recs;
  }
  // The two teardowns.  leave_closed(): the device memory goes back BEFORE the process leaves (0.15 s for the 200 GB a 30x
  // sample maps), not with the kernel's teardown of an exited process: the tool that runs next starts sooner (DESIGN.md
  // section 4.11 has the measurements).  RFX_LEAVE_NO_CLOSE=1: as it was.
  void leave_closed() {
    if (!getenv("RFX_LEAVE_NO_CLOSE")) {
      for (rfx_ctx* c : ctxs) rfx_close(c);
      trace("count: device closed");
    }
    leave(0);
  }
  void close(const std::vector<rfx_records*>& recs) {  // --timing, RFX_CLEAN_EXIT=1: everything handed back piece by piece
    for (rfx_records* r : recs) rfx_records_free(r);
    for (rfx_table* tb : tabs) rfx_count_free(tb);
    if (peers) rfx_peers_free(peers);
    for (rfx_ctx* c : ctxs) rfx_close(c);
    trace("count: closed");
  }
};

// One run: what survey() finds out about the inputs, and what the routes share.
struct CountRun {
  const CountArgs& a;
  CountDevices dv;
  std::vector<Input> inputs;
  size_t known_bytes = 0;
  bool any_stream = false;
  unsigned nthreads = 1;  // parser threads
  OutputPrealloc prealloc;
  double prealloc_frac = 0.19;  // RFX_PREALLOC_FRAC / RFX_PREALLOC_MIN: the tests reach both sides of the guess
  size_t prealloc_min = 256u << 20;
  const bool sync_open = getenv("RFX_SYNC_OPEN") != nullptr;  // (A/B: the device opened before anything else, as until round 6)
  ReadBatch batch;  // the sequential parser's reads
  PackedBatch packed;
  std::unique_ptr<CountIngest> ingest;  // (kept to the end: its page-locked blocks serve the output drain)
  std::unique_ptr<TextIngest> text;
  std::unique_ptr<BgzfIngest> bgzf, fasta;
  std::unique_ptr<GzipIngest> gzip;
  std::unique_ptr<BamIngest> bam;
  CountRun(const CountArgs& a_, const std::vector<int>& gpus) : a(a_), dv(gpus) {}
  std::function<void(rfx_reads*)> sink() { return [this](rfx_reads* r) { dv.sink_to(0, r); }; }  // (the device-side routes: one device)
};

// Every input opened and sized, and what follows from that, before a device is asked for: an open and an fstat per input.
static void survey(CountRun& run) {
  const CountArgs& a = run.a;
  for (const char* path : a.inputs) {
    Input in{path, strcmp(path, "stdin") == 0 || strcmp(path, "/dev/stdin") == 0 ? 0 : ::open(path, O_RDONLY), false, 0};
    if (in.fd < 0) die(std::string("Failed to open input file '") + path + "'");
    struct stat st;
    if (fstat(in.fd, &st) == 0 && S_ISREG(st.st_mode)) {
      in.regular = true;
      in.size = (size_t)st.st_size;
      run.known_bytes += in.size;
    } else {
      run.any_stream = true;
    }
    run.inputs.push_back(in);
  }
  if (a.keep_path && a.bam_chr && run.inputs.size() != 1)
    die("rufus_amd jellyfish count: --bam --keep-packed goes with ONE input: the cache describes one file's records");
  if (a.keep_path && !a.bam_chr && (!a.sam_chr || run.inputs.size() != 1))
    die("rufus_amd jellyfish count: --keep-packed goes with --sam and ONE input (a pipe with --spool, or a SAM file)");
  if (a.keep_path && run.any_stream && !a.spool_path)  // (the cache points into the stream: without a copy of it there is nothing to point into)
    die("rufus_amd jellyfish count: --keep-packed of a piped input needs --spool FILE (the cache refers to lines of the stream)");
  if (a.spool_path && (!run.any_stream || run.inputs.size() != 1))
    die("rufus_amd jellyfish count: --spool copies ONE piped input; a regular file can be given to the next stage as it is");
  run.nthreads = std::min((unsigned)std::max(1, a.threads), rfx_host_cpus());  // -t 40 on a 16-CPU cgroup: 16 parsers
  if (const char* ev = getenv("RFX_HOST_THREADS")) run.nthreads = (unsigned)std::max(1, atoi(ev));
  const bool msp_ok = a.k >= 23 && a.k <= 31;  // the super-k-mer path (rfx_count_set_passes needs it)
  run.dv.defer = msp_ok && (run.any_stream || run.known_bytes > (16ull << 30) || getenv("RFX_COUNT_PASSES"));
  if (const char* ev = getenv("RFX_COUNT_DEFER")) run.dv.defer = msp_ok && atoi(ev) != 0;
  if (run.dv.n() > 1) run.dv.defer = true;
}

// ~11 bytes of output per distinct solid k-mer: 0.18 of the FASTQ bytes at 30x, less on shallow or filtered input
static void start_prealloc(CountRun& run) {
  if (const char* ev = getenv("RFX_PREALLOC_MIN")) run.prealloc_min = (size_t)strtoull(ev, nullptr, 10);
  if (const char* ev = getenv("RFX_PREALLOC_FRAC")) run.prealloc_frac = atof(ev);
  if (getenv("RFX_NO_PREALLOC")) return;
  if (!run.any_stream && run.known_bytes > run.prealloc_min)
    run.prealloc.start(run.a.out, (uint64_t)((double)run.known_bytes * run.prealloc_frac));
  // a piped input (scripts/RunJellyForRUFUS.sh:28: samtools view | ... | jellyfish count /dev/fd/0): the guess follows
  // the bytes that have come in (profiles/r03_cli_w_trio.txt: 8.5 s of page faults after the device had finished)
  else if (run.any_stream && run.inputs.size() == 1)
    run.prealloc.start_growing(run.a.out);
}

enum class Route { BAM, BGZF_FASTQ, BGZF_FASTA, GZIP, DEVICE_TEXT, HOST_PARALLEL, SEQUENTIAL };

// Does the BGZF file begin with a BAM header?  (rfx_bam_header refuses BGZF whose first bytes are not BAM's magic; a header
// that is not whole in the first 64 KiB is still BAM.)  What turns `jellyfish count X.bam` without --bam into a message
// that says --bam instead of the FASTQ one.
static bool is_bam(int fd, uint64_t size) {
  if (!rfx_bam_header) return false;
  const std::vector<uint8_t> head = read_head(fd, size, 1u << 16);
  int complete = 0;
  int32_t n_ref = 0;
  uint64_t names_bytes = 0, first_block = 0;
  uint32_t skip = 0;
  return rfx_bam_header(head.data(), head.size(), &complete, &n_ref, nullptr, 0, &names_bytes, &first_block, &skip) == RFX_OK;
}
// Plain gzip is inflated on the device by default since it was measured against the pipe on a whole sample (DESIGN.md
// section 4.20: 5.4 s against 58 s); RFX_GZIP_DEVICE=0 sends plain gzip where it went before.
static bool gzip_on_device() { return !(getenv("RFX_GZIP_DEVICE") && atoi(getenv("RFX_GZIP_DEVICE")) == 0); }

// Which route an input takes, or why it takes none.  Every input decides for itself, by these tests in this order.
static Route route_of(const CountArgs& a, const Input& in, int n_gpu, unsigned nthreads) {
  if (a.bam_chr) {  // every input is a BAM file: one device, a regular file, neither --sam nor --spool
    if (!in.regular) die("rufus_amd jellyfish count: --bam needs a regular file, not a pipe: the BAM is mapped");
    if (!is_bgzf(in.fd, in.regular, in.size)) die(std::string("rufus_amd jellyfish count: --bam: '") + in.path + "' is not BGZF");
    return Route::BAM;
  }
  const bool alone = n_gpu == 1 && a.plain();  // what the routes that inflate or parse on the device need
  if (is_bgzf(in.fd, in.regular, in.size)) {  // (rfx_cli.hpp)
    if (is_bam(in.fd, in.size))
      die(std::string("rufus_amd jellyfish count: '") + in.path + "' is a BAM file: count it with --bam CHR_FILE");
    if (!alone)
      die("rufus_amd jellyfish count: BGZF input is inflated on the device, which needs one device and none of --sam, "
          "--spool, --keep-packed: inflate it and pipe it in");
    // a first inflated byte '>' is a reference FASTA (`ref.fa.gz` as `samtools faidx` wants it), anything else is taken for FASTQ
    return bgzf_first_byte(in.fd, in.size) == '>' ? Route::BGZF_FASTA : Route::BGZF_FASTQ;
  }
  if (gzip_on_device() && is_plain_gzip(in.fd, in.regular, in.size)) {  // (rfx_cli.hpp)
    if (!alone)
      die("rufus_amd jellyfish count: plain-gzip input is inflated on the device, which needs one device and none of --sam, "
          "--spool, --keep-packed: inflate it and pipe it in");
    if (gzip_first_byte(in.fd, in.size) != '@')
      die(std::string("rufus_amd jellyfish count: '") + in.path + "' is plain gzip and its first inflated byte is not '@': only "
          "FASTQ is inflated on the device; pipe anything else in through zcat");
    return Route::GZIP;
  }
  // RFX_DEVICE_PARSE=1 (kernel K1): a regular FASTQ file's text is parsed and packed on the device (rfx_ingest.hpp TextIngest,
  // csrc/rfx_text.hip).  Not the default: with 16 parser threads a draw (profiles/r06_text_route.txt).
  if (alone && nthreads > 1 && getenv("RFX_DEVICE_PARSE") && !getenv("RFX_HOST_PARSE") && in.regular && in.size > 0)
    return Route::DEVICE_TEXT;
  return nthreads > 1 || !a.plain() ? Route::HOST_PARALLEL : Route::SEQUENTIAL;
}

static int open_side_file(const char* what, const char* path) {  // the --keep-packed cache, the --spool copy
  const int fd = ::open(path, O_WRONLY | O_CREAT | O_TRUNC, 0644);
  if (fd < 0) die(std::string("Can't open ") + what + " '" + path + "'");
  return fd;
}

// a regular input of the BAM, BGZF and gzip routes: mapped, fed whole, unmapped, the route's counts traced
template <typename R>
static void feed_whole(R& route, Input& in) {
  const Mapped m = map_regular(in.fd, true);
  if (!m.ok) die(std::string("cannot map '") + in.path + "': " + strerror(errno));
  route.feed_mapped(m.p, m.n);
  munmap((void*)m.p, m.n);
  trace(("count: " + route.counts()).c_str());
}

// --bam (rfx_ingest.hpp BamIngest); --keep-packed with the one input leaves the BAM-kind cache (rfx_bam_cache.hpp)
static void route_bam(CountRun& run, Input& in) {
  const CountArgs& a = run.a;
  if (!run.bam) {
    Opener::wait();
    run.bam.reset(new BamIngest(run.dv.ctxs[0], run.sink(), a.bam_exclude, env_arena("RFX_BAM_ARENA"), env_piece((size_t)8 << 20)));
    if (a.keep_path) run.bam->set_keep_packed(open_side_file("the packed-read cache", a.keep_path), a.keep_minq);
    if (a.bam_region) run.bam->set_region(a.bam_region, in.path);
    trace("count: bam route, arenas open");
  }
  feed_whole(*run.bam, in);
  if (a.keep_path) {  // (one input: checked by survey()) the file is a cache only from here on
    run.bam->finish_keep_packed();
    trace(("count: " + run.bam->keep_counts()).c_str());
  }
}

// A bgzip'd FASTQ is inflated, parsed and packed on the device (rfx_ingest.hpp BgzfIngest; csrc/rfx_bgzf.hip) whether or not
// RFX_DEVICE_PARSE is set: compressed, the text is ~80 bytes per read over PCIe and the host only reads the file.  Replaces
// `zcat F.fastq.gz | ...` (runRufus.sh:157-160).  A bgzip'd FASTA takes the same route with the FASTA carry and parse
// (csrc/rfx_fasta.hip): replaces the `zcat ref.fa.gz |` in front of the -e / -f databases (runRufus.sh:77, :115).
static void route_bgzf(CountRun& run, Input& in, bool fasta) {
  std::unique_ptr<BgzfIngest>& route = fasta ? run.fasta : run.bgzf;
  if (!route) {
    Opener::wait();
    // (the FASTQ mode has no arena knob; RFX_FASTA_ARENA: >= 1 MiB, < 4 GiB)
    route.reset(new BgzfIngest(run.dv.ctxs[0], run.sink(), env_arena(fasta ? "RFX_FASTA_ARENA" : nullptr, 1ll << 20, ARENA_MAX),
                               env_piece((size_t)8 << 20), fasta));
    trace(fasta ? "count: fasta route, text arenas open" : "count: bgzf route, text arenas open");
  }
  feed_whole(*route, in);
}

// A plain-gzip FASTQ is inflated on the device too (rfx_ingest.hpp GzipIngest; csrc/rfx_gzip.hip: the stream cut
// speculatively, a chain rule on the host).  Replaces `zcat F.fastq.gz | ...` (runRufus.sh:157-160, :229-232).
static void route_gzip(CountRun& run, Input& in) {
  if (!run.gzip) {
    Opener::wait();
    run.gzip.reset(new GzipIngest(run.dv.ctxs[0], run.sink(), env_arena("RFX_GZIP_ARENA", 1ll << 20, ARENA_MAX), env_piece((size_t)128 << 20)));
    trace("count: gzip route, text arenas open");
  }
  feed_whole(*run.gzip, in);
}

static void flush(CountRun& run) {
  if (run.batch.n() == 0) return;
  const int rc = run.packed.pack(run.batch, RFX_PACK_COUNT, 0);
  if (rc) die(std::string("rufus_amd: pack failed: ") + rfx_strerror(rc));
  run.dv.to_all([&](rfx_ctx* c) { return run.packed.upload(c, run.batch.n(), RFX_PACK_COUNT); });
  run.batch.clear();
}
// the reference's grammar: FASTA, multi-line FASTQ
static void sequential(CountRun& run, LineReader& lr) {
  const bool ok = parse_sequences(lr, [&](const char* s, size_t n) {
    run.batch.add(s, n);
    if (run.batch.seq.size() >= (256u << 20) || run.batch.n() >= (1u << 22)) flush(run);
  });
  if (!ok) die("Unsupported format");
  flush(run);  // k-mers never span files
}
// the input from its descriptor, behind what a parallel parser had already read of it
static void route_sequential(CountRun& run, Input& in, const std::vector<char>& head) {
  LineReader lr;
  if (!head.empty()) lr.preload(head.data(), head.size());
  lr.attach(in.fd);
  in.fd = -1;  // closed by the reader
  sequential(run, lr);
}

// false: the device refused the file; the host parser takes it
static bool route_device_text(CountRun& run, Input& in) {
  if (!run.text) {
    Opener::wait();
    run.text.reset(new TextIngest(
        run.dv.ctxs[0], run.nthreads, run.sink(),
        [&run](const char* text, size_t n) {  // refused by the device (not strict 4-line FASTQ): the reference's grammar
          LineReader lr(n + (1u << 20));
          lr.preload(text, n);
          lr.close_input();
          sequential(run, lr);
        },
        (size_t)1 << 30, env_piece((size_t)8 << 20)));
    trace("count: text arenas open, copiers up");
  }
  bool done = false;
  if (getenv("RFX_TEXT_PREAD")) {  // (the workers pread their ranges: 0.69 against 0.92 s per 20 GB, much slower for three at once)
    done = run.text->feed_file(in.fd, in.size);
    trace("count: text fed");
  } else if (const Mapped m = map_regular(in.fd, true); m.ok) {
    done = run.text->feed_mapped(m.p, m.n);
    trace("count: text fed");
    munmap((void*)m.p, m.n);
    trace("count: input unmapped");
  }
  return done;
}

// The parallel host parser (rfx_ingest.hpp CountIngest) on a file or a pipe.  false: it refused the file, or the pipe's head
// (`head`: what it had read of the pipe by then); the sequential parser takes the input -- unless --spool forbids that.
static bool route_host_parallel(CountRun& run, Input& in, std::vector<char>& head) {
  const CountArgs& a = run.a;
  if (!run.ingest) {
    run.ingest.reset(new CountIngest(
        run.nthreads,
        [&run](const StageBlock& b) {
          run.dv.to_all([&](rfx_ctx* c) { return rfx_reads_upload(c, b.codes, b.acgt, nullptr, b.word_off, b.len, b.n_reads); });
        },
        run.sync_open ? rfx_host_alloc : rfx_host_alloc_lazy, rfx_host_free, 4u << 20, 24ull << 20, run.sync_open ? nullptr : rfx_host_pin));
    run.ingest->set_sam(a.sam_chr != nullptr);
    if (a.spool_path) run.ingest->set_spool(open_side_file("spool file", a.spool_path));
    if (a.keep_path) run.ingest->set_keep_packed(open_side_file("the packed-read cache", a.keep_path), a.keep_minq);
    if (getenv("RFX_INGEST_PIECE")) run.ingest->set_piece_bytes(env_piece(0));
    if (run.prealloc.growing())
      run.ingest->on_stream_bytes = [&run](uint64_t so_far) {
        if (so_far > run.prealloc_min) run.prealloc.want((uint64_t)((double)so_far * run.prealloc_frac));
      };
    trace("count: staging blocks pinned, workers up");
  }
  if (in.regular) {
    if (in.size == 0) return true;
    // mapped, not pread: measured on the 256-core box (20 GB FASTQ in tmpfs, 64 workers) 1.1 s against 3.2 s
    // with every worker pread-ing its range into a private buffer (RFX_INGEST_PREAD=1 keeps that path testable)
    if (getenv("RFX_INGEST_PREAD") && !a.sam_chr) return run.ingest->feed_file(in.fd, in.size);
    const Mapped m = map_regular(in.fd, true);
    if (!m.ok) return false;
    const bool done = run.ingest->feed_mapped(m.p, m.n);
    munmap((void*)m.p, m.n);
    return done;
  }
  head.resize(1u << 16);
  size_t got = 0;
  while (got < head.size()) {
    const ssize_t n = ::read(in.fd, head.data() + got, head.size() - got);
    if (n < 0 && errno == EINTR) continue;
    if (n < 0) die(std::string("read error on input: ") + strerror(errno));
    if (n == 0) break;
    got += (size_t)n;
  }
  head.resize(got);
  if (gzip_on_device() && got >= 3 && (unsigned char)head[0] == 0x1f && (unsigned char)head[1] == 0x8b && head[2] == 0x08)
    die("rufus_amd jellyfish count: gzip input needs a regular file, not a pipe: the file is mapped; or inflate it and pipe the text in");
  const bool done = got == 0 || run.ingest->feed_stream(in.fd, head);
  if (!done && a.spool_path) die("rufus_amd jellyfish count: --spool needs SAM (--sam) or strict 4-line FASTQ on the pipe");
  return done;
}

// One input down its route.  Device text that refuses a file falls through to the host parser, a host parser that refuses
// a file or a pipe's head to the sequential one.
static void feed(CountRun& run, Input& in) {
  std::vector<char> head;
  switch (route_of(run.a, in, run.dv.n(), run.nthreads)) {
    case Route::BAM: route_bam(run, in); break;
    case Route::BGZF_FASTQ: route_bgzf(run, in, false); break;
    case Route::BGZF_FASTA: route_bgzf(run, in, true); break;
    case Route::GZIP: route_gzip(run, in); break;
    case Route::DEVICE_TEXT:
      if (route_device_text(run, in)) break;
      [[fallthrough]];
    case Route::HOST_PARALLEL:
      if (route_host_parallel(run, in, head)) break;
      [[fallthrough]];
    case Route::SEQUENTIAL: route_sequential(run, in, head);
  }
  if (in.fd > 0) ::close(in.fd);
}

// src/PassThroughSamCheck.cpp:37-44: the names the route logged, or, when no input took the route, its "notachr"
template <typename R>
static void write_chr_log(const char* path, const std::unique_ptr<R>& route) {
  FILE* cf = fopen(path, "w");
  if (!cf) {
    printf("ERROR, Output file could not be opened -%s\n", path);
    return;
  }
  if (route)
    for (const std::string& name : route->chr_log()) fprintf(cf, "%s\n", name.c_str());
  else fprintf(cf, "notachr\n");
  fclose(cf);
}

// The caches and logs of the fed inputs closed, the device-side routes' arenas handed back.
static void close_routes(CountRun& run) {
  const CountArgs& a = run.a;
  // the packed-read cache is a cache only from here on: its header now says how many chunks describe how long a stream
  if (a.keep_path && run.ingest) run.ingest->finish_keep_packed(run.inputs[0].regular ? run.inputs[0].size : run.ingest->spooled_bytes());
  if (a.bam_chr) write_chr_log(a.bam_chr, run.bam);
  run.bam.reset();
  if (a.sam_chr) write_chr_log(a.sam_chr, run.ingest);
  run.bgzf.reset();
  run.fasta.reset();
  run.gzip.reset();
}

static void trace_pages(const char* fmt, uint64_t x, uint64_t y, uint64_t z = 0) {  // (fmt: two or three %llu; only when traced)
  if (!getenv("RFX_CLI_TRACE")) return;
  char msg[160];
  snprintf(msg, sizeof msg, fmt, (unsigned long long)x, (unsigned long long)y, (unsigned long long)z);
  trace(msg);
}

static int count_main(int argc, char** argv, int full_argc, char** full_argv) {
  const double t_start = now();
  CountArgs a;
  parse_count(argc, argv, a);
  // RUFUS_GPUS needs the super-k-mer path (23 <= k <= 31): else the first device alone
  std::vector<int> gpus = gpu_list();
  if (gpus.size() > 1 && !(a.k >= 23 && a.k <= 31)) {
    fprintf(stderr, "rufus_amd jellyfish: k = %d is counted on one device (RUFUS_GPUS needs 23 <= k <= 31)\n", a.k);
    gpus.resize(1);
  }
  CountRun run(a, gpus);
  survey(run);
  Opener opener([&run] { run.dv.open(run.a); });
  const double t_init = now();
  start_prealloc(run);
  if (run.sync_open) Opener::wait();
  if (a.bam_chr && run.dv.n() != 1) die(BAM_ALONE);
  for (Input& in : run.inputs) feed(run, in);
  close_routes(run);
  // (device-parsed input: no staging blocks to lend to the output drain -- its ring of page-locked buffers is made now,
  // beside the device's finish, instead of in front of the first write)
  std::vector<std::pair<char*, size_t>> out_ring;
  std::thread out_ring_pinner;
  if (!run.ingest && run.text) {
    trace(("count: text route, " + run.text->timing()).c_str());
    run.text.reset();  // (its page-locked text buffers go first)
    out_ring_pinner = std::thread([&out_ring] {
      for (int i = 0; i < 8; ++i)
        if (char* p = (char*)rfx_host_alloc(48u << 20)) out_ring.emplace_back(p, (size_t)48u << 20);
    });
  }
  opener.join();  // (an empty input: nobody asked for the device yet)
  const double t_count = now();
  trace("count: input parsed and queued");
  trace_pages("write: output pages wanted %llu, allocated %llu, in the page table %llu", run.prealloc.wanted(), run.prealloc.reached(),
              run.prealloc.populated());

  // RFX_COUNT_HISTO=1 (opt-in, not jellyfish behaviour): also write OUT.histo, byte for byte what `jellyfish histo -f -o OUT.histo OUT`
  // would: scripts/RunJellyForRUFUS.sh:36-38 runs histo only when that file is missing (a 35 GB re-read saved per sample).
  std::vector<uint64_t> hist(getenv("RFX_COUNT_HISTO") ? RFX_HISTO_BINS : 0);
  const std::vector<rfx_records*> recs = run.dv.finish(a.lower, a.upper, hist.empty() ? nullptr : hist.data());
  std::vector<uint64_t> cols(2 * (size_t)a.k);
  rfx_jf_matrix(a.lsize, a.k, cols.data());
  if (!hist.empty())
    if (FILE* hf = fopen((std::string(a.out) + ".histo").c_str(), "w")) {
      for (int i = 0; i < RFX_HISTO_BINS; ++i) fprintf(hf, "%d %llu\n", i, (unsigned long long)hist[(size_t)i]);
      fclose(hf);
    }
  const int out_fd = run.prealloc.take();
  trace_pages("write: %llu bytes preallocated, %llu in the mapping's page table", run.prealloc.reached(), run.prealloc.populated());
  if (out_ring_pinner.joinable()) out_ring_pinner.join();
  write_jhash(a.out, recs, cols.data(), a.canonical, a.out_counter_len, full_argc, full_argv,
              run.ingest ? run.ingest->lend_buffers(48u << 20) : out_ring, out_fd, run.prealloc.reached(), run.prealloc.take_mapping());
  trace("count: output closed");
  if (!a.timing && !getenv("RFX_CLEAN_EXIT")) run.dv.leave_closed();
  run.ingest.reset();
  for (auto& b : out_ring) rfx_host_free(b.first);
  run.dv.close(recs);
  if (FILE* f = a.timing ? fopen(a.timing, "w") : nullptr) {
    fprintf(f, "Init     %g\nCounting %g\nWriting  %g\n", t_init - t_start, t_count - t_init, now() - t_count);
    fclose(f);
  }
  return 0;
}

// ---------------------------------------------------------------------------------------------
static int histo_main(int argc, char** argv) {
  bool full = false;
  const char* out = nullptr;
  uint64_t low = 1, high = 10000, inc = 1;
  static option lo[] = {{"full", 0, 0, 'f'}, {"output", 1, 0, 'o'}, {"low", 1, 0, 'l'},      {"high", 1, 0, 'h'},
                        {"increment", 1, 0, 'i'}, {"threads", 1, 0, 't'}, {0, 0, 0, 0}};
  optind = 1;
  int ch;
  while ((ch = getopt_long(argc, argv, "fo:l:h:i:t:", lo, nullptr)) != -1) {
    switch (ch) {
      case 'f': full = true; break;
      case 'o': out = optarg; break;
      case 'l': parse_si(optarg, low); break;
      case 'h': parse_si(optarg, high); break;
      case 'i': parse_si(optarg, inc); break;
      case 't': break;
      default: die("Usage: jellyfish histo [-f] [-o OUT] db");
    }
  }
  if (optind >= argc) die("Missing database");
  if (low != 1 || high != 10000 || inc != 1)
    die("rufus_amd jellyfish histo: only the default --low 1 --high 10000 --increment 1 is supported");
  rfx_ctx* ctx = open_ctx();
  trace("histo: device open");
  std::vector<uint64_t> hist(RFX_HISTO_BINS, 0);
  rfx_records* rec = nullptr;
  JhashFile db;
  if (!db.open(argv[optind])) {  // not a regular file: loaded whole
    JhashHeader h;
    rec = load_records(ctx, argv[optind], h);
    if (rfx_records_histo(rec, hist.data()) != RFX_OK) die(std::string("rufus_amd: ") + rfx_last_error());
  } else {  // 256 M records (5 GB of HBM) at a time, whatever the size of the database
    uint64_t per = 256ull << 20;
    if (const char* ev = getenv("RFX_HISTO_SLICE_RECORDS")) per = std::max<uint64_t>(1, strtoull(ev, nullptr, 10));
    std::vector<uint64_t> part_hist(RFX_HISTO_BINS);
    for (uint64_t at = 0; at < db.n; at += per) {
      rfx_records* part = db.load(ctx, at, std::min(db.n, at + per));
      if (rfx_records_histo(part, part_hist.data()) != RFX_OK) die(std::string("rufus_amd: ") + rfx_last_error());
      for (int i = 0; i < RFX_HISTO_BINS; ++i) hist[(size_t)i] += part_hist[(size_t)i];
      rfx_records_free(part);
    }
  }
  trace("histo: counted");
  FILE* f = out ? fopen(out, "w") : stdout;
  if (!f) die(std::string("Error opening output file '") + out + "'");
  for (int i = 0; i < RFX_HISTO_BINS; ++i)  // jf/sub_commands/histo_main.cc:82-84
    if (hist[(size_t)i] > 0 || full) fprintf(f, "%d %llu\n", i, (unsigned long long)hist[(size_t)i]);
  if (out) fclose(f);
  leave(0);
  db.close();
  if (rec) rfx_records_free(rec);
  rfx_close(ctx);
  return 0;
}

// ---------------------------------------------------------------------------------------------
// `jellyfish query [-s FASTA]... DB [mers...]` (jf/sub_commands/query_main.cc:44-51,:110-115), and, SURVEY row N3:
// SEVERAL databases in one call -- `jellyfish query -s FA -o OUT1 -o OUT2 -o OUT3 DB1 DB2 DB3` writes to OUTi exactly
// the lines `jellyfish query -s FA DBi` prints.  scripts/Overlap.shorter.sh:265-299 looks the same two k-mer lists up in
// the subject's and every control's 30x database with one process each (scripts/CheckJellyHashList.sh:12); here the
// k-mers are parsed, canonicalised and dealt to position ranges once, the device is opened once, and of every database
// only the ranges that got a k-mer are read.  (One -o, or none, with several databases: one line per k-mer with a
// count column per database.)  A positional argument after the first that names an existing file is a database.
static int query_main(int argc, char** argv) {
  std::vector<const char*> seq_files, outs;
  static option lo[] = {{"sequence", 1, 0, 's'}, {"output", 1, 0, 'o'}, {"load", 0, 0, 'l'}, {"no-load", 0, 0, 'L'},
                        {0, 0, 0, 0}};
  optind = 1;
  int ch;
  while ((ch = getopt_long(argc, argv, "s:o:lL", lo, nullptr)) != -1) {
    switch (ch) {
      case 's': seq_files.push_back(optarg); break;
      case 'o': outs.push_back(optarg); break;
      case 'l': case 'L': break;
      default: die("Usage: jellyfish query [-s FASTA] [-o OUT]... db [db...] [mers...]");
    }
  }
  if (optind >= argc) die("Missing database");
  std::vector<const char*> db_paths{argv[optind]}, mers;
  // (the reference takes `db mers...`; further databases are an extension -- an argument spelt like a mer stays a mer
  // even if the working directory holds a file of that name)
  auto looks_like_mer = [](const char* a) {
    const size_t n = strlen(a);
    if (n == 0 || n > 32) return false;
    for (size_t i = 0; i < n; ++i)
      if (!strchr("ACGTacgt", a[i])) return false;
    return true;
  };
  for (int i = optind + 1; i < argc; ++i) {
    if (!looks_like_mer(argv[i]) && ::access(argv[i], R_OK) == 0) db_paths.push_back(argv[i]);
    else mers.push_back(argv[i]);
  }
  const size_t n_db = db_paths.size();
  if (outs.size() > 1 && outs.size() != n_db) die("jellyfish query: one -o per database (or a single one)");
  rfx_ctx* ctx = open_ctx();
  std::vector<JhashFile> dbs(n_db);
  std::vector<rfx_records*> whole(n_db, nullptr);
  std::vector<bool> sliced(n_db, false);
  for (size_t d = 0; d < n_db; ++d) {
    sliced[d] = dbs[d].open(db_paths[d]);
    if (!sliced[d]) whole[d] = load_records(ctx, db_paths[d], dbs[d].h);  // (a pipe: header and payload in one pass)
    if (dbs[d].h.k != dbs[0].h.k || dbs[d].h.canonical != dbs[0].h.canonical)
      die("jellyfish query: the databases of one call must have the same mer length and canonical flag");
  }
  const JhashHeader& h = dbs[0].h;
  const int k = h.k;
  const uint64_t kmask = k == 32 ? ~0ull : ((1ull << (2 * k)) - 1);
  std::vector<uint64_t> keys;
  // every k-mer of the query sequences (jf/sub_commands/query_main.cc:44-51), canonicalised when the
  // database is (:115); the lookups themselves run on the device
  for (const char* path : seq_files) {
    LineReader in;
    if (!in.open(path)) die(std::string("Failed to open input file '") + path + "'");
    const bool ok = parse_sequences(in, [&](const char* s, size_t n) {
      uint64_t fwd = 0, rc = 0;
      int filled = 0;
      for (size_t i = 0; i < n; ++i) {
        uint64_t one;
        if (!text_to_key(s + i, 1, one)) { filled = 0; continue; }
        fwd = ((fwd << 2) | one) & kmask;
        rc = (rc >> 2) | ((3 - one) << (2 * (k - 1)));
        if (filled < k) ++filled;
        if (filled >= k) keys.push_back(h.canonical && rc < fwd ? rc : fwd);
      }
    });
    if (!ok) die("Unsupported format");
  }
  for (const char* m : mers) {  // query_from_cmdline
    uint64_t key;
    if ((int)strlen(m) != k || !text_to_key(m, (size_t)k, key)) {
      fprintf(stderr, "Invalid mer '%s'\n", m);
      continue;
    }
    keys.push_back(h.canonical ? std::min(key, revcomp_key(key, k)) : key);
  }
  if (keys.size() > 0xFFFFFFFFull) die("rufus_amd jellyfish query: too many k-mers in one call");
  std::vector<std::vector<uint32_t>> counts(n_db, std::vector<uint32_t>(keys.size() + 1, 0));
  std::vector<uint64_t> key_pos;  // position of every query, computed once per hash function:
  int key_pos_lsize = -1;         // the function key_pos holds now -- NOT that of the database before this one, which
  std::vector<uint64_t> key_pos_cols;  // may have been piped or empty and never have touched key_pos
  for (size_t d = 0; d < n_db; ++d) {
    const JhashHeader& hd = dbs[d].h;
    JhashFile& db = dbs[d];
    if (!sliced[d]) {
      if (rfx_query(whole[d], keys.data(), keys.size(), counts[d].data()) != RFX_OK) die(std::string("rufus_amd: ") + rfx_last_error());
      continue;
    }
    if (keys.empty() || !db.n) continue;
    // The database stays on disk: it is cut into position ranges of ~64 M records (RFX_QUERY_SLICE_RECORDS), the
    // queries are dealt to the ranges by their own position, and only ranges that got queries are read -- a few
    // hundred MB of HBM whatever the database size.
    uint64_t per = 64ull << 20;
    if (const char* ev = getenv("RFX_QUERY_SLICE_RECORDS")) per = std::max<uint64_t>(1, strtoull(ev, nullptr, 10));
    const uint64_t S = std::max<uint64_t>(1, (db.n + per - 1) / per);
    if (key_pos.size() != keys.size() || hd.lsize != key_pos_lsize || hd.cols != key_pos_cols) {
      key_pos.resize(keys.size());
      for (size_t i = 0; i < keys.size(); ++i) key_pos[i] = rfx_jf_pos(hd.cols.data(), hd.k, hd.lsize, keys[i]);
      key_pos_lsize = hd.lsize;
      key_pos_cols.assign(hd.cols.begin(), hd.cols.end());
    }
    // (a located position costs ~30 single-record reads, a streamed record 0.3 ns: worth it below one query per few
    // thousand records -- RFX_QUERY_SPARSE_RATIO, default 4096)
    uint64_t sparse_ratio = 4096;
    if (const char* ev = getenv("RFX_QUERY_SPARSE_RATIO")) sparse_ratio = std::max<uint64_t>(1, strtoull(ev, nullptr, 10));
    if (keys.size() * sparse_ratio < db.n && !getenv("RFX_QUERY_NO_SPARSE")) {
      // Few k-mers against a big database (the hash-list lookup of runRufus.sh:925-926: thousands against 10^8..10^10
      // records): every position range would get one, i.e. the whole file would travel.  Instead the records AT the
      // queried positions are located on the host (a binary search per distinct position over the sorted file -- what
      // binary_dumper.hpp:156-203 does for every lookup), read, and uploaded as one small sorted database; the lookups
      // still run on the device.
      std::vector<uint64_t> ps(key_pos);
      std::sort(ps.begin(), ps.end());
      ps.erase(std::unique(ps.begin(), ps.end()), ps.end());
      std::vector<std::pair<uint64_t, uint64_t>> rg(ps.size());
      const unsigned nt = std::max(1u, std::min(16u, rfx_host_cpus()));
      std::vector<std::thread> th;
      for (unsigned t = 0; t < nt; ++t)
        th.emplace_back([&, t] {
          for (size_t j = t; j < ps.size(); j += nt) {
            const uint64_t i0 = db.lower_bound_pos(ps[j]);
            uint64_t i1 = i0;
            while (i1 < db.n && db.pos_at(i1) == ps[j]) ++i1;
            rg[j] = {i0, i1};
          }
        });
      for (auto& x : th) x.join();
      uint64_t tot = 0;
      for (auto& r : rg) tot += r.second - r.first;
      if (tot == 0) continue;  // nothing stored at any queried position: every count is 0
      std::vector<char> buf((size_t)tot * db.rl);
      size_t at = 0;
      for (auto& r : rg) {
        size_t want = (size_t)(r.second - r.first) * db.rl, got = 0;
        while (got < want) {
          const ssize_t w = ::pread(db.fd, buf.data() + at + got, want - got, (off_t)(hd.payload_offset + r.first * db.rl + got));
          if (w < 0 && errno == EINTR) continue;
          if (w <= 0) die("read error on '" + db.path + "'");
          got += (size_t)w;
        }
        at += want;
      }
      rfx_records* part = rfx_records_load(ctx, hd.k, hd.lsize, hd.cols.data(), buf.data(), tot, hd.counter_len);
      if (!part) die("rufus_amd: cannot load '" + db.path + "': " + rfx_last_error());
      if (rfx_query(part, keys.data(), keys.size(), counts[d].data()) != RFX_OK) die(std::string("rufus_amd: ") + rfx_last_error());
      rfx_records_free(part);
      continue;
    }
    std::vector<std::vector<uint32_t>> in_slice(S);
    for (size_t i = 0; i < keys.size(); ++i) in_slice[slice_of(key_pos[i], S, hd.lsize)].push_back((uint32_t)i);
    std::vector<uint64_t> sub;
    std::vector<uint32_t> got;
    for (uint64_t sidx = 0; sidx < S; ++sidx) {
      if (in_slice[sidx].empty()) continue;
      const uint64_t i0 = sidx == 0 ? 0 : db.lower_bound_pos(slice_start(sidx, S, hd.lsize));
      const uint64_t i1 = sidx + 1 == S ? db.n : db.lower_bound_pos(slice_start(sidx + 1, S, hd.lsize));
      if (i1 == i0) continue;  // an empty range: its queries count 0
      rfx_records* part = db.load(ctx, i0, i1);
      sub.clear();
      for (uint32_t qi : in_slice[sidx]) sub.push_back(keys[qi]);
      got.assign(sub.size() + 1, 0);
      if (rfx_query(part, sub.data(), sub.size(), got.data()) != RFX_OK) die(std::string("rufus_amd: ") + rfx_last_error());
      for (size_t j = 0; j < sub.size(); ++j) counts[d][in_slice[sidx][j]] = got[j];
      rfx_records_free(part);
    }
  }
  if (outs.size() > 1) {  // one file per database: the lines a one-database call prints
    for (size_t d = 0; d < n_db; ++d) {
      FILE* f = fopen(outs[d], "w");
      if (!f) die(std::string("Error opening output file '") + outs[d] + "'");
      for (size_t i = 0; i < keys.size(); ++i) fprintf(f, "%s %u\n", key_to_text(keys[i], k).c_str(), counts[d][i]);
      fclose(f);
    }
  } else {
    FILE* f = outs.empty() ? stdout : fopen(outs[0], "w");
    if (!f) die(std::string("Error opening output file '") + outs[0] + "'");
    for (size_t i = 0; i < keys.size(); ++i) {
      fputs(key_to_text(keys[i], k).c_str(), f);
      for (size_t d = 0; d < n_db; ++d) fprintf(f, " %u", counts[d][i]);
      fputc('\n', f);
    }
    if (!outs.empty()) fclose(f);
  }
  leave(0);
  for (size_t d = 0; d < n_db; ++d) {
    dbs[d].close();
    if (whole[d]) rfx_records_free(whole[d]);
  }
  rfx_close(ctx);
  return 0;
}

// ---------------------------------------------------------------------------------------------
static int dump_main(int argc, char** argv) {
  bool column = false, tab = false;
  const char* out = nullptr;
  uint64_t lower = 0, upper = std::numeric_limits<uint64_t>::max();
  static option lo[] = {{"column", 0, 0, 'c'},      {"tab", 0, 0, 't'},         {"lower-count", 1, 0, 'L'},
                        {"upper-count", 1, 0, 'U'}, {"output", 1, 0, 'o'},      {0, 0, 0, 0}};
  optind = 1;
  int ch;
  while ((ch = getopt_long(argc, argv, "ctL:U:o:", lo, nullptr)) != -1) {
    switch (ch) {
      case 'c': column = true; break;
      case 't': tab = true; break;
      case 'L': parse_si(optarg, lower); break;
      case 'U': parse_si(optarg, upper); break;
      case 'o': out = optarg; break;
      default: die("Usage: jellyfish dump [-c] [-t] [-L n] [-U n] [-o OUT] db");
    }
  }
  if (optind >= argc) die("Missing database");
  rfx_ctx* ctx = open_ctx();
  JhashHeader h;
  rfx_records* rec = load_records(ctx, argv[optind], h);
  const uint64_t n = rfx_records_size(rec);
  std::vector<uint64_t> keys(n + 1);
  std::vector<uint32_t> counts(n + 1);
  if (rfx_records_get(rec, keys.data(), counts.data(), nullptr) != RFX_OK) die(std::string("rufus_amd: ") + rfx_last_error());
  FILE* f = out ? fopen(out, "w") : stdout;
  if (!f) die(std::string("Error opening output file '") + out + "'");
  for (uint64_t i = 0; i < n; ++i) {  // jf/sub_commands/dump_main.cc:36-53
    if (counts[i] < lower || counts[i] > upper) continue;
    if (column) fprintf(f, "%s%c%u\n", key_to_text(keys[i], h.k).c_str(), tab ? '\t' : ' ', counts[i]);
    else fprintf(f, ">%u\n%s\n", counts[i], key_to_text(keys[i], h.k).c_str());
  }
  if (out) fclose(f);
  leave(0);
  rfx_records_free(rec);
  rfx_close(ctx);
  return 0;
}

// ---------------------------------------------------------------------------------------------
static int merge_main(int argc, char** argv, int full_argc, char** full_argv) {
  const char* out = "mer_counts_merged.jf";
  static option lo[] = {{"output", 1, 0, 'o'}, {"lower-count", 1, 0, 'L'}, {"upper-count", 1, 0, 'U'}, {0, 0, 0, 0}};
  optind = 1;
  int ch;
  while ((ch = getopt_long(argc, argv, "o:L:U:", lo, nullptr)) != -1) {
    if (ch == 'o') out = optarg;
    else if (ch != 'L' && ch != 'U') die("Usage: jellyfish merge [-o OUT] db1 db2 ...");
  }
  if (optind >= argc) die("Missing database");
  rfx_ctx* ctx = open_ctx();
  const int nf = argc - optind;
  std::vector<JhashFile> jf((size_t)nf);
  std::vector<JhashHeader> hs((size_t)nf);
  std::vector<rfx_records*> whole((size_t)nf, nullptr);  // inputs that are not regular files: loaded as before
  bool all_sliced = true;
  for (int i = 0; i < nf; ++i) {
    if (!jf[(size_t)i].open(argv[optind + i])) {
      all_sliced = false;
      whole[(size_t)i] = load_records(ctx, argv[optind + i], hs[(size_t)i]);
    } else {
      hs[(size_t)i] = jf[(size_t)i].h;
    }
  }
  for (size_t i = 1; i < hs.size(); ++i) {  // jf/jellyfish/merge_files.cc:193-203
    if (hs[i].k != hs[0].k) die("Can't merge hashes of different key lengths");
    if (hs[i].lsize != hs[0].lsize) die("Can't merge hash with different size");
    if (hs[i].cols != hs[0].cols) die("Can't merge hash with different hash function");
  }
  // formatted by hand: printf + std::string per line is 10x slower, and the list can have 1e8 lines
  std::vector<char> line((size_t)1 << 20);
  auto emit = [&](const uint64_t* keys, const uint32_t* counts, uint64_t n) {
    size_t fill = 0;
    const int kk = hs[0].k;
    for (uint64_t i = 0; i < n; ++i) {
      if (fill + (size_t)kk + 16 > line.size()) {
        fwrite(line.data(), 1, fill, stdout);
        fill = 0;
      }
      for (int b = 0; b < kk; ++b) line[fill++] = "ACGT"[(keys[i] >> (2 * (kk - 1 - b))) & 3u];
      line[fill++] = '\t';
      char dig[12];
      int nd = 0;
      uint32_t v = counts[i];
      do { dig[nd++] = (char)('0' + v % 10); v /= 10; } while (v);
      while (nd) line[fill++] = dig[--nd];
      line[fill++] = '\n';
    }
    fwrite(line.data(), 1, fill, stdout);
  };
  // The result is a small part of the inputs (k-mers private to one sample): room for 64 M of them first, the
  // exact number -- which a short call reports -- if that was not enough.  (Sizing by the inputs would be 115 GB
  // of host memory for a 30x trio.)
  std::vector<uint64_t> keys;
  std::vector<uint32_t> counts;
  auto merge_and_emit = [&](const std::vector<rfx_records*>& files) {
    uint64_t total = 0, n = 0;
    for (auto* r : files) total += rfx_records_size(r);
    uint64_t cap = std::min<uint64_t>(total, 64ull << 20);
    if (keys.size() < cap + 1) keys.resize(cap + 1), counts.resize(cap + 1);
    int rc = rfx_merge_unique(ctx, files.data(), (int)files.size(), 5, keys.data(), counts.data(), cap, &n);
    if (rc == RFX_E_RANGE && n > cap) {
      cap = n;
      keys.resize(cap + 1);
      counts.resize(cap + 1);
      rc = rfx_merge_unique(ctx, files.data(), (int)files.size(), 5, keys.data(), counts.data(), cap, &n);
    }
    if (rc) die(std::string("rufus_amd: merge failed: ") + rfx_strerror(rc) + " " + rfx_last_error());
    emit(keys.data(), counts.data(), n);
  };
  if (!all_sliced) {
    for (int i = 0; i < nf; ++i)
      if (!whole[(size_t)i]) whole[(size_t)i] = jf[(size_t)i].load(ctx, 0, jf[(size_t)i].n);
    merge_and_emit(whole);
  } else {
    // A merge-path join over position ranges (the files are sorted by position first): range by range, the part
    // of every input that falls into it is read, joined on the device and printed -- ranges come in increasing
    // order, so the output is the same sorted list.  ~2.4e9 records (48 GB of HBM) per range: one range for
    // anything small, 5 for a 30x trio (RFX_MERGE_SLICES overrides; a range costs ~0.6 s of fixed work: three 30x
    // samples of a 1 Gb genome, 3.1e9 records, merge in 1.8 s as one range and in 3.6 s as three).
    uint64_t total = 0;
    for (auto& f : jf) total += f.n;
    uint64_t S = std::max<uint64_t>(1, (total + 2399999999ull) / 2400000000ull);
    if (const char* ev = getenv("RFX_MERGE_SLICES")) S = std::max<uint64_t>(1, strtoull(ev, nullptr, 10));
    std::vector<uint64_t> lo((size_t)nf, 0);
    for (uint64_t sidx = 0; sidx < S; ++sidx) {
      std::vector<rfx_records*> part((size_t)nf, nullptr);
      for (int i = 0; i < nf; ++i) {
        const JhashFile& f = jf[(size_t)i];
        const uint64_t hi = sidx + 1 == S ? f.n : f.lower_bound_pos(slice_start(sidx + 1, S, hs[0].lsize));
        part[(size_t)i] = f.load(ctx, lo[(size_t)i], hi);
        lo[(size_t)i] = hi;
      }
      trace("merge: a position range of every input loaded");
      merge_and_emit(part);
      for (auto* r : part) rfx_records_free(r);
      trace("merge: joined and printed");
    }
  }
  fflush(stdout);
  // the reference leaves a header-only database behind (merge_files.cc:207-224; testRun/clean.sh:1 removes it)
  std::vector<char> hdr(1 << 16);
  const long hl = rfx_jhash_header(hs[0].k, hs[0].lsize, hs[0].cols.data(), hs[0].canonical, hs[0].counter_len,
                                   full_argc, full_argv, hdr.data(), hdr.size());
  if (hl > 0)
    if (FILE* f = fopen(out, "wb")) {
      fwrite(hdr.data(), 1, (size_t)hl, f);
      fclose(f);
    }
  leave(0);
  for (auto* r : whole)
    if (r) rfx_records_free(r);
  for (auto& f : jf) f.close();
  rfx_close(ctx);
  return 0;
}

int main(int argc, char** argv) {
  trace("main");
  if (argc < 2) die("Usage: jellyfish <count|histo|query|dump|merge> [options]");
  const std::string cmd = argv[1];
  if (cmd == "count") return count_main(argc - 1, argv + 1, argc, argv);
  if (cmd == "histo") return histo_main(argc - 1, argv + 1);
  if (cmd == "query") return query_main(argc - 1, argv + 1);
  if (cmd == "dump") return dump_main(argc - 1, argv + 1);
  if (cmd == "merge") return merge_main(argc - 1, argv + 1, argc, argv);
  if (cmd == "--version" || cmd == "-V") {
    printf("jellyfish 2.2.5 (rufus_amd drop-in: %s)\n", rfx_version());
    return 0;
  }
  die("Unknown sub-command '" + cmd + "' (rufus_amd provides count, histo, query, dump, merge)");
}
