// K1 ("read 2-bit pack + validity mask"): strict 4-line FASTQ TEXT -> a packed read block, on the device.
//
// The reference parses text with one producer thread per file (jf/include/jellyfish/mer_overlap_sequence_parser.hpp:
// 179-206: header line, sequence line, '+' line, quality line) and packs bases as the hashing threads consume them
// (jf/include/jellyfish/mer_dna.hpp:46-63).  Until round 6 the drop-in `jellyfish count` did both on the host -- parse
// and AVX2 pack at ~1 us per read and thread -- and uploaded 68 bytes per read; on the GPU box's 16-CPU quota that was
// most of a count's wall time while the device sat idle.  Here the host only moves bytes: record-aligned pieces of the
// text are appended to a device arena (rfx_text_append: one H2D copy each, from pinned memory), and rfx_text_parse turns
// the arena into a read block:
//
//   k_txt_count   newlines per 4 KB tile (exact SWAR zero-byte count of text ^ '\n')          -> scan -> tile ranks
//   k_txt_lines   line_start[i + 1] = the byte after the i-th newline (a 256-thread scan per tile)
//   k_txt_reads   record r = lines 4r .. 4r+3: checks the shape ('@' line, '+' line, quality as long as the sequence),
//                 len[r], words of the read; block totals (bases, longest read, reads shorter than 32) by atomics
//                                                                                            -> scan -> word offsets
//   k_txt_pack    one thread per code word: 32 bases -> 64 bits of jellyfish codes + the ACGT mask (RFX_PACK_COUNT), or
//                 RUFUS codes + the good mask from the quality line (RFX_PACK_FILTER) -- rfx_pack_reads' tables
//
// Anything that is not strict 4-line FASTQ (blank lines between records, multi-line records, a truncated tail) makes
// rfx_text_parse report "not strict" and the caller parses that text on the host, as before (rfx_text_fetch hands it
// back): the device path never guesses.  Two waits per block (line count, then word count): ~50 us against the 20 ms a
// gigabyte of text takes over PCIe.
//
// bgzip'd text (rfx_text_append_bgzf, replaces runRufus.sh:157-160's `zcat`): the compressed blocks are copied to a staging
// area of the arena and k_bgzf_inflate (rfx_bgzf.hip) writes their text into the arena; BGZF blocks end anywhere, so
// rfx_text_settle cuts the arena at its last whole group of four lines (k_txt_count again, then k_txt_nth finds the byte
// behind newline number 4 * floor(N / 4)) and carries the tail into the next arena.
//
// Two bgzip'd mate files in lock step (replaces runRufus.sh:974-977's `<(zcat A) <(zcat B)`): two arenas filled from two
// files hold different numbers of whole records, so rfx_text_records reports an arena's floor(N / 4) and
// rfx_text_settle_records -- rfx_text_settle's body -- cuts at a record count the caller gives (the smaller of the two).
// rfx_gather.hip copies the text of selected records out of an arena; it finds the lines through rfxi::text_* below.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "rfx_bgzf_core.h"
#include "rfx_internal.h"

using rfxi::dfree;
using rfxi::dmalloc;
using rfxi::queue_read;

namespace {

int hip_fail(hipError_t e, const char* what) {
  char msg[256];
  snprintf(msg, sizeof msg, "%s: %s", what, hipGetErrorString(e));
  rfxi::set_error(msg);
  return RFX_E_HIP;
}
hipError_t ctx_sync(rfx_ctx* c) { return rfxi::sync(c); }
#define HIPCHK(x)                                   \
  do {                                              \
    hipError_t e_ = (x);                            \
    if (e_ != hipSuccess) return hip_fail(e_, #x);  \
  } while (0)

constexpr int TX_TILE = 4096, TX_BLOCK = 256;  // 16 bytes per thread

struct txt_stats {
  unsigned long long n_bases, n_words;
  unsigned int bad, max_len, lower_cgt;
  unsigned int short_cnt[32];
};

__device__ __forceinline__ uint32_t nl_bits(uint32_t x) {  // bit 7 of every byte that is '\n', exactly
  const uint32_t y = x ^ 0x0A0A0A0Au;
  const uint32_t t = (y & 0x7F7F7F7Fu) + 0x7F7F7F7Fu;
  return ~(t | y | 0x7F7F7F7Fu);
}

__global__ __launch_bounds__(TX_BLOCK) void k_txt_count(const uint4* __restrict__ text, uint64_t n_tiles,
                                                         uint64_t* __restrict__ tile_cnt) {
  __shared__ uint32_t s_sum;
  for (uint64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    if (threadIdx.x == 0) s_sum = 0;
    __syncthreads();
    const uint4 v = text[tile * (TX_TILE / 16) + threadIdx.x];
    uint32_t c = __popc(nl_bits(v.x)) + __popc(nl_bits(v.y)) + __popc(nl_bits(v.z)) + __popc(nl_bits(v.w));
#pragma unroll
    for (int o = 32; o; o >>= 1) c += __shfl_xor(c, o);
    if ((threadIdx.x & 63) == 0) atomicAdd(&s_sum, c);
    __syncthreads();
    if (threadIdx.x == 0) tile_cnt[tile] = s_sum;
    __syncthreads();
  }
}

__global__ __launch_bounds__(TX_BLOCK) void k_txt_lines(const uint4* __restrict__ text, uint64_t n_tiles,
                                                         const uint64_t* __restrict__ tile_off,
                                                         uint32_t* __restrict__ line_start, uint64_t max_lines) {
  __shared__ uint32_t s_wave[TX_BLOCK / 64];
  for (uint64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const uint4 v = text[tile * (TX_TILE / 16) + threadIdx.x];
    const uint32_t b[4] = {nl_bits(v.x), nl_bits(v.y), nl_bits(v.z), nl_bits(v.w)};
    const uint32_t c = __popc(b[0]) + __popc(b[1]) + __popc(b[2]) + __popc(b[3]);
    uint32_t incl = c;  // inclusive scan over the wave, then over the four waves
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const uint32_t up = __shfl_up(incl, d, 64);
      if ((int)(threadIdx.x & 63u) >= d) incl += up;
    }
    if ((threadIdx.x & 63u) == 63u) s_wave[threadIdx.x >> 6] = incl;
    __syncthreads();
    uint32_t before = incl - c;
    for (uint32_t w = 0; w < (threadIdx.x >> 6); ++w) before += s_wave[w];
    uint64_t rank = tile_off[tile] + before;
    const uint32_t pos0 = (uint32_t)(tile * TX_TILE) + threadIdx.x * 16u;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      uint32_t m = b[q];
      while (m) {
        const int bit = __ffs((int)m) - 1;  // 7, 15, 23, 31
        m &= m - 1u;
        // (line_start has max_lines + 1 entries: rfx_text_gather sizes it by the caller's record count, not by the text)
        if (++rank <= max_lines) line_start[rank] = pos0 + (uint32_t)q * 4u + (uint32_t)(bit >> 3) + 1u;
      }
    }
    __syncthreads();
  }
}

// *cut = the byte offset behind newline number `want` (1-based, want <= the text's newlines): ONE workgroup; tile_off is
// the exclusive scan of k_txt_count's counts (tile_off[n_tiles] = all newlines).
__global__ __launch_bounds__(TX_BLOCK) void k_txt_nth(const uint4* __restrict__ text, uint64_t n_tiles,
                                                       const uint64_t* __restrict__ tile_off, uint64_t want,
                                                       uint64_t* __restrict__ cut) {
  __shared__ uint32_t s_wave[TX_BLOCK / 64];
  uint64_t lo = 0, hi = n_tiles;  // the tile with tile_off[tile] < want <= tile_off[tile + 1]
  while (hi - lo > 1) {
    const uint64_t mid = (lo + hi) / 2;
    if (tile_off[mid] < want) lo = mid;
    else hi = mid;
  }
  const uint64_t tile = lo;
  const uint4 v = text[tile * (TX_TILE / 16) + threadIdx.x];
  const uint32_t b[4] = {nl_bits(v.x), nl_bits(v.y), nl_bits(v.z), nl_bits(v.w)};
  const uint32_t c = __popc(b[0]) + __popc(b[1]) + __popc(b[2]) + __popc(b[3]);
  uint32_t incl = c;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t up = __shfl_up(incl, d, 64);
    if ((int)(threadIdx.x & 63u) >= d) incl += up;
  }
  if ((threadIdx.x & 63u) == 63u) s_wave[threadIdx.x >> 6] = incl;
  __syncthreads();
  uint32_t before = incl - c;
  for (uint32_t w = 0; w < (threadIdx.x >> 6); ++w) before += s_wave[w];
  uint64_t rank = tile_off[tile] + before;  // newlines in front of this thread's 16 bytes
  if (rank < want && want <= rank + c) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      uint32_t m = b[q];
      while (m) {
        const int bit = __ffs((int)m) - 1;  // 7, 15, 23, 31
        m &= m - 1u;
        if (++rank == want) *cut = tile * TX_TILE + threadIdx.x * 16u + (uint32_t)q * 4u + (uint32_t)(bit >> 3) + 1u;
      }
    }
  }
}

// rfx_pack_reads' tables (rfx_host.cpp PackLut): jellyfish code of either case / RUFUS code of upper case only
__device__ __forceinline__ bool is_acgt_upper(uint32_t ch) { return ch == 'A' || ch == 'C' || ch == 'G' || ch == 'T'; }
__device__ __forceinline__ uint32_t base_code(uint32_t ch) {  // of an A/C/G/T in either case: A0 C1 G2 T3
  const uint32_t x = (ch >> 1) & 3u;
  return x ^ (x >> 1);
}

__global__ __launch_bounds__(256) void k_txt_reads(const uint8_t* __restrict__ text, const uint32_t* __restrict__ line_start,
                                                    uint64_t n_reads, uint32_t* __restrict__ len, uint64_t* __restrict__ words,
                                                    txt_stats* __restrict__ st) {
  for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n_reads; r += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t l0 = line_start[4 * r], l1 = line_start[4 * r + 1], l2 = line_start[4 * r + 2], l3 = line_start[4 * r + 3],
                   l4 = line_start[4 * r + 4];
    const uint32_t L = l2 - 1u - l1, Q = l4 - 1u - l3;
    // (an empty header or '+' line cannot be: a line that starts with the marker has a byte)
    const bool ok = l1 - l0 >= 2u && text[l0] == '@' && l3 - l2 >= 2u && text[l2] == '+' && L == Q;
    if (!ok) atomicOr(&st->bad, 1u);
    len[r] = L;
    words[r] = (L + 31u) / 32u;
    atomicAdd(&st->n_bases, (unsigned long long)L);  // (one per read: 4 M atomics per block of text, ~0.2 ms)
    atomicMax(&st->max_len, L);
    if (L < 32u) atomicAdd(&st->short_cnt[L], 1u);
  }
}

// One thread per (read, word): MAXW words per read are walked, a read has the first ceil(len / 32) of them.
template <bool FILTER>
__global__ __launch_bounds__(256) void k_txt_pack(const uint8_t* __restrict__ text, const uint32_t* __restrict__ line_start,
                                                   const uint64_t* __restrict__ word_off64, const uint32_t* __restrict__ len,
                                                   uint64_t n_reads, uint32_t maxw, int min_q, uint64_t* __restrict__ codes,
                                                   uint32_t* __restrict__ mask, uint32_t* __restrict__ word_off,
                                                   txt_stats* __restrict__ st) {
  const uint64_t total = n_reads * maxw;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t r = i / maxw;
    const uint32_t wi = (uint32_t)(i - r * maxw);
    const uint32_t L = len[r];
    const uint64_t w0 = word_off64[r];
    if (wi == 0) word_off[r] = (uint32_t)w0;
    if (r == n_reads - 1 && wi == 0) word_off[n_reads] = (uint32_t)word_off64[n_reads];
    if (wi * 32u >= L) continue;
    const uint32_t nb = min(32u, L - wi * 32u);
    const uint8_t* s = text + line_start[4 * r + 1] + wi * 32u;
    const uint8_t* q = FILTER ? text + line_start[4 * r + 3] + wi * 32u : nullptr;
    uint64_t c = 0;
    uint32_t m = 0;
    bool lower = false;
    for (uint32_t b = 0; b < nb; ++b) {
      const uint32_t ch = s[b];
      if (FILTER) {  // src/Util.cpp:51-84: upper-case ACGT, anything else encodes as A; src/RUFUS.Filter.cpp:205: the good mask
        if (is_acgt_upper(ch)) c |= (uint64_t)base_code(ch) << (2 * b);
        const int qv = (int)(signed char)q[b];  // (the reference's plain `char`: a byte above 127 is a negative quality)
        if (!(qv - 33 < min_q || ch == 'N')) m |= 1u << b;
        lower |= ch == 'c' || ch == 'g' || ch == 't';
      } else if (is_acgt_upper(ch & 0xDFu)) {  // jf mer_dna.hpp:46-63: either case
        c |= (uint64_t)base_code(ch) << (2 * b);
        m |= 1u << b;
      }
    }
    codes[w0 + wi] = c;
    mask[w0 + wi] = m;
    if (FILTER && lower) atomicOr(&st->lower_cgt, 1u);
  }
}

}  // namespace

struct rfx_text {
  rfx_ctx* ctx = nullptr;
  uint8_t* arena = nullptr;
  uint64_t cap = 0, used = 0;
  bool vmm = false;
  // The copies run on a stream of their own: text for the NEXT block crosses PCIe while this ctx's stream parses and
  // counts the block before it (a second rfx_text of the same ctx) -- on the ctx stream copies and kernels would take
  // turns.  rfx_text_parse makes the ctx stream wait for the last copy.
  hipStream_t copy = nullptr;
  std::mutex mu;               // append / copied / wait may come from several host threads (the ingest's workers)
  // One event per append: its bytes have left the host buffer.  The events live until close and are recorded again by
  // the appends after a reset (n_ev of them are this generation's): a waiter that still holds a handle from before the
  // reset -- whose copy is long done: the reset follows the parse -- must find an event, not freed memory.
  std::vector<hipEvent_t> ev;
  size_t n_ev = 0;
  // ---- BGZF appends (rfx_text_append_bgzf) ----
  // The kernel runs on a second stream behind the append's copies (an event between them), so the inflate of one append
  // overlaps the copy of the next; whoever reads the arena synchronises with both streams first (bgzf_check).
  hipStream_t kern = nullptr;
  hipEvent_t staged = nullptr;
  // Staging: compressed bytes + 8 bytes of padding, descriptors and status words of every append since the reset, bump-
  // allocated from chunks that are kept across resets (one chunk once the first arena's worth has been seen).
  struct stage_chunk { uint8_t* p; size_t cap, used; };
  std::vector<stage_chunk> stage;
  struct bgzf_append { uint32_t first, n; uint32_t* status; };
  std::vector<bgzf_append> bgzf;               // this generation's BGZF appends: block indices [first, first + n)
  std::vector<std::vector<bgzf_desc>> descs;   // (their descriptors: the host side of an asynchronous copy)
  uint32_t n_bgzf_blocks = 0;
  uint32_t* first_bad = nullptr;  // device: the lowest index of a block that failed, or ~0
  bool bgzf_failed = false;
  std::string bgzf_msg;
  rfxi::text_bam bam;  // rfx_bam.hip: the record starts of the last rfx_bam_settle, kept until the reset
};

namespace {

uint8_t* stage_alloc(rfx_text* t, size_t bytes) {  // (t->mu held) 16-byte aligned
  bytes = (bytes + 15) & ~(size_t)15;
  for (auto& ch : t->stage)
    if (ch.cap - ch.used >= bytes) {
      uint8_t* p = ch.p + ch.used;
      ch.used += bytes;
      return p;
    }
  // a chunk holds what a quarter of the arena deflates to at 4 : 1 several times over; a bigger append gets its own
  const size_t cap = std::max<size_t>(bytes, std::min<size_t>((size_t)t->cap / 4 + (1u << 20), (size_t)256 << 20));
  uint8_t* p = nullptr;
  if (hipMalloc((void**)&p, cap) != hipSuccess) {
    (void)hipGetLastError();
    return nullptr;
  }
  t->stage.push_back({p, cap, bytes});
  return p;
}

// RFX_OK, or RFX_E_FORMAT with "rfx_bgzf: block <index in this arena>: <reason>" as the error text: a block appended
// since the last reset did not inflate.  Waits for the arena's copies and kernels.
int bgzf_check(rfx_text* t) {
  if (!t->n_bgzf_blocks) return RFX_OK;
  if (!t->bgzf_failed) {
    HIPCHK(hipStreamSynchronize(t->copy));
    HIPCHK(hipStreamSynchronize(t->kern));
    uint32_t bad = ~0u;
    HIPCHK(hipMemcpy(&bad, t->first_bad, 4, hipMemcpyDeviceToHost));
    if (bad == ~0u) return RFX_OK;
    uint32_t st = 0;
    for (const auto& a : t->bgzf)
      if (bad >= a.first && bad - a.first < a.n) HIPCHK(hipMemcpy(&st, a.status + (bad - a.first), 4, hipMemcpyDeviceToHost));
    char msg[160];
    snprintf(msg, sizeof msg, "rfx_bgzf: block %u: %s", bad, bgzf_status_text(st));
    t->bgzf_msg = msg;
    t->bgzf_failed = true;
  }
  rfxi::set_error(t->bgzf_msg.c_str());
  return RFX_E_FORMAT;
}

}  // namespace

// ---- what rfx_gather.hip needs of an arena ---------------------------------------------------------------------------
namespace rfxi {

int text_ready(rfx_text* t, rfx_ctx** c, const uint8_t** arena, uint64_t* used) {
  (void)hipSetDevice(t->ctx->device);
  HIPCHK(hipStreamSynchronize(t->copy));
  if (t->kern) HIPCHK(hipStreamSynchronize(t->kern));
  if (const int rc = bgzf_check(t)) return rc;
  *c = t->ctx;
  *arena = t->arena;
  *used = t->used;
  return RFX_OK;
}

int text_claim(rfx_text* t, rfx_ctx** c, uint8_t** arena, uint64_t* cap, uint64_t* used) {
  const uint8_t* a = nullptr;
  if (const int rc = text_ready(t, c, &a, used)) return rc;
  *arena = t->arena;
  *cap = t->cap;
  return RFX_OK;
}
void text_grow(rfx_text* t, uint64_t n) {
  std::lock_guard<std::mutex> g(t->mu);
  t->used += n;
}

rfx_ctx* text_ctx(rfx_text* t) { return t->ctx; }
text_bam& text_bam_of(rfx_text* t) { return t->bam; }

int text_cut(rfx_text* t, rfx_text* next, uint64_t cut, uint64_t* carried, const char* who) {
  rfx_ctx* c = t->ctx;
  const uint64_t n = t->used;
  const uint64_t tail = n - cut;
  if (tail) {
    if (!next) {
      rfxi::set_error((std::string(who) + ": the text ends inside a record").c_str());
      return RFX_E_FORMAT;
    }
    if (tail > next->cap) return RFX_E_RANGE;
    HIPCHK(hipMemcpyAsync(next->arena, t->arena + cut, tail, hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(ctx_sync(c));
    std::lock_guard<std::mutex> g(next->mu);
    next->used = tail;
  }
  t->used = cut;
  *carried = tail;
  return RFX_OK;
}

hipError_t text_count_lines(rfx_ctx* c, const uint8_t* arena, uint64_t n, uint64_t* tile_off) {
  // whole tiles are read: what lies behind the text holds no newline (the arena has 2 * TX_TILE bytes behind its capacity)
  const hipError_t e = hipMemsetAsync(const_cast<uint8_t*>(arena) + n, 0, 2 * TX_TILE, c->stream);
  if (e != hipSuccess) return e;
  const uint64_t n_tiles = (n + TX_TILE - 1) / TX_TILE;
  const int grid = (int)std::min<uint64_t>(n_tiles, (uint64_t)c->n_cu * 8);
  {
    rfx_span sp(c, "k_txt_count");
    hipLaunchKernelGGL(k_txt_count, dim3(grid), dim3(TX_BLOCK), 0, c->stream, (const uint4*)arena, n_tiles, tile_off);
  }
  rfxk::scan_tail(c, tile_off, n_tiles);
  return hipGetLastError();
}

hipError_t text_line_starts(rfx_ctx* c, const uint8_t* arena, uint64_t n, const uint64_t* tile_off, uint32_t* line_start,
                            uint64_t max_lines) {
  const hipError_t e = hipMemsetAsync(line_start, 0, 4, c->stream);
  if (e != hipSuccess) return e;
  const uint64_t n_tiles = (n + TX_TILE - 1) / TX_TILE;
  const int grid = (int)std::min<uint64_t>(n_tiles, (uint64_t)c->n_cu * 8);
  rfx_span sp(c, "k_txt_lines");
  hipLaunchKernelGGL(k_txt_lines, dim3(grid), dim3(TX_BLOCK), 0, c->stream, (const uint4*)arena, n_tiles, tile_off, line_start,
                     max_lines);
  return hipGetLastError();
}

}  // namespace rfxi

extern "C" {

rfx_text* rfx_text_open(rfx_ctx* c, uint64_t cap_bytes) {
  if (!c || cap_bytes == 0 || cap_bytes > (0xFFFFFFFFull - 2 * TX_TILE)) return nullptr;  // (32-bit line offsets)
  (void)hipSetDevice(c->device);
  rfx_text* t = new rfx_text();
  t->ctx = c;
  t->cap = cap_bytes;
  // (plain hipMalloc, not the ctx's arena of mapped virtual memory: RFX_TEXT_VMM=1 keeps the arena for the A/B)
  t->vmm = getenv("RFX_TEXT_VMM") != nullptr;
  if (t->vmm) {
    t->arena = (uint8_t*)dmalloc(c, (size_t)cap_bytes + 2 * TX_TILE);
    if (t->arena && ctx_sync(c) != hipSuccess) { dfree(c, t->arena); t->arena = nullptr; }
  } else if (hipMalloc((void**)&t->arena, (size_t)cap_bytes + 2 * TX_TILE) != hipSuccess) {
    (void)hipGetLastError();
    t->arena = nullptr;
  }
  if (!t->arena || hipStreamCreateWithFlags(&t->copy, hipStreamNonBlocking) != hipSuccess) {
    if (t->arena) { if (t->vmm) dfree(c, t->arena); else (void)hipFree(t->arena); }
    delete t;
    return nullptr;
  }
  return t;
}

void rfx_text_close(rfx_text* t) {
  if (!t) return;
  (void)hipSetDevice(t->ctx->device);
  (void)hipStreamSynchronize(t->copy);
  if (t->kern) {
    (void)hipStreamSynchronize(t->kern);
    (void)hipStreamDestroy(t->kern);
    (void)hipEventDestroy(t->staged);
    (void)hipFree(t->first_bad);
  }
  dfree(t->ctx, t->bam.rec_start);
  dfree(t->ctx, t->bam.region);
  for (auto& ch : t->stage) (void)hipFree(ch.p);
  for (hipEvent_t e : t->ev) (void)hipEventDestroy(e);
  (void)hipStreamDestroy(t->copy);
  if (t->vmm) dfree(t->ctx, t->arena);
  else (void)hipFree(t->arena);
  delete t;
}

uint64_t rfx_text_room(const rfx_text* t) { return t ? t->cap - t->used : 0; }
uint64_t rfx_text_bytes(const rfx_text* t) { return t ? t->used : 0; }

long rfx_text_append(rfx_text* t, const void* host, uint64_t n) {
  if (!t || (!host && n)) return RFX_E_INVAL;
  rfx_ctx* c = t->ctx;
  (void)hipSetDevice(c->device);
  std::lock_guard<std::mutex> g(t->mu);
  if (n > t->cap - t->used) return RFX_E_RANGE;
  if (t->n_ev == t->ev.size()) {
    hipEvent_t e;
    if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) return RFX_E_HIP;
    t->ev.push_back(e);
  }
  hipError_t rc = n ? hipMemcpyAsync(t->arena + t->used, host, n, hipMemcpyHostToDevice, t->copy) : hipSuccess;
  if (rc == hipSuccess) rc = hipEventRecord(t->ev[t->n_ev], t->copy);
  if (rc != hipSuccess) return hip_fail(rc, "rfx_text_append");
  t->used += n;
  return (long)t->n_ev++;
}

static int text_event(rfx_text* t, long ticket, hipEvent_t* e) {
  std::lock_guard<std::mutex> g(t->mu);
  if (ticket < 0 || (size_t)ticket >= t->n_ev) return RFX_E_INVAL;
  *e = t->ev[(size_t)ticket];
  return RFX_OK;
}

int rfx_text_copied(rfx_text* t, long ticket) {
  hipEvent_t e;
  if (!t || text_event(t, ticket, &e) != RFX_OK) return RFX_E_INVAL;
  const hipError_t rc = hipEventQuery(e);
  if (rc == hipSuccess) return 1;
  if (rc == hipErrorNotReady) {
    (void)hipGetLastError();
    return 0;
  }
  return hip_fail(rc, "rfx_text_copied");
}

int rfx_text_wait(rfx_text* t, long ticket) {
  hipEvent_t e;
  if (!t || text_event(t, ticket, &e) != RFX_OK) return RFX_E_INVAL;
  (void)hipSetDevice(t->ctx->device);
  HIPCHK(hipEventSynchronize(e));
  return RFX_OK;
}

int rfx_text_fetch(rfx_text* t, void* host) {
  if (!t || !host) return RFX_E_INVAL;
  rfx_ctx* c = t->ctx;
  (void)hipSetDevice(c->device);
  HIPCHK(hipStreamSynchronize(t->copy));
  if (const int rc = bgzf_check(t)) return rc;
  if (t->used) HIPCHK(hipMemcpyAsync(host, t->arena, t->used, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(ctx_sync(c));
  return RFX_OK;
}

void rfx_text_reset(rfx_text* t) {
  if (!t) return;
  (void)hipSetDevice(t->ctx->device);
  (void)hipStreamSynchronize(t->copy);
  if (t->kern) (void)hipStreamSynchronize(t->kern);
  std::lock_guard<std::mutex> g(t->mu);
  t->n_ev = 0;
  t->used = 0;
  if (t->bam.rec_start) dfree(t->ctx, t->bam.rec_start);
  if (t->bam.region) dfree(t->ctx, t->bam.region);
  t->bam = rfxi::text_bam();
  if (t->n_bgzf_blocks) {
    if (t->stage.size() > 1) {  // one chunk of the size that was needed, next time
      size_t all = 0;
      for (auto& ch : t->stage) { all += ch.used; (void)hipFree(ch.p); }
      t->stage.clear();
      uint8_t* p = nullptr;
      if (hipMalloc((void**)&p, all) == hipSuccess) t->stage.push_back({p, all, 0});
      else (void)hipGetLastError();
    }
    for (auto& ch : t->stage) ch.used = 0;
    t->bgzf.clear();
    t->descs.clear();
    t->n_bgzf_blocks = 0;
    t->bgzf_failed = false;
    (void)hipMemset(t->first_bad, 0xFF, 4);
  }
}

long rfx_text_append_bgzf(rfx_text* t, const void* host, uint64_t n) {
  if (!t || (!host && n)) return RFX_E_INVAL;
  rfx_ctx* c = t->ctx;
  (void)hipSetDevice(c->device);
  uint32_t nb = 0;
  uint64_t consumed = 0, inflated = 0;
  const int src = rfx_bgzf_scan(host, n, 0xFFFFFFFFu, &nb, &consumed, &inflated);
  if (src != RFX_OK || consumed != n) {
    rfxi::set_error("rfx_text_append_bgzf: not a run of whole BGZF blocks");
    return RFX_E_FORMAT;
  }
  std::lock_guard<std::mutex> g(t->mu);
  if (inflated > t->cap - t->used || (uint64_t)t->n_bgzf_blocks + nb > 0xFFFFFFF0ull) return RFX_E_RANGE;
  if (!t->kern) {
    if (hipStreamCreateWithFlags(&t->kern, hipStreamNonBlocking) != hipSuccess) { t->kern = nullptr; return hip_fail(hipGetLastError(), "rfx_text_append_bgzf"); }
    hipError_t e = hipEventCreateWithFlags(&t->staged, hipEventDisableTiming);
    if (e == hipSuccess) e = hipMalloc((void**)&t->first_bad, 4);
    if (e == hipSuccess) e = hipMemset(t->first_bad, 0xFF, 4);
    if (e != hipSuccess) return hip_fail(e, "rfx_text_append_bgzf");
  }
  if (t->n_ev == t->ev.size()) {
    hipEvent_t e;
    if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) return RFX_E_HIP;
    t->ev.push_back(e);
  }
  // descriptors: every block's payload inside the staged bytes, its text inside the arena's room (checked above)
  t->descs.emplace_back(nb);
  std::vector<bgzf_desc>& ds = t->descs.back();
  const uint8_t* b = (const uint8_t*)host;
  uint64_t at = 0, out = t->used;
  for (uint32_t i = 0; i < nb; ++i) {
    uint32_t bsize, pay_off, pay_len, isize, crc;
    (void)bgzf_block_header(b + at, n - at, &bsize, &pay_off, &pay_len, &isize, &crc);  // (the scan accepted it)
    ds[i] = bgzf_desc{at + pay_off, out, pay_len, isize, crc, 0};
    at += bsize;
    out += isize;
  }
  // (a failure below gives back what this call took: the descriptors and the staging bytes)
  std::vector<size_t> marks;
  for (const auto& ch : t->stage) marks.push_back(ch.used);
  auto undo = [&] {
    while (t->stage.size() > marks.size()) {
      (void)hipFree(t->stage.back().p);
      t->stage.pop_back();
    }
    for (size_t i = 0; i < marks.size(); ++i) t->stage[i].used = marks[i];
    t->descs.pop_back();
  };
  uint8_t* d_in = nb ? stage_alloc(t, (size_t)n + 8) : nullptr;  // 8 bytes of padding behind the compressed bytes
  bgzf_desc* d_desc = nb ? (bgzf_desc*)stage_alloc(t, (size_t)nb * sizeof(bgzf_desc)) : nullptr;
  uint32_t* d_status = nb ? (uint32_t*)stage_alloc(t, (size_t)nb * 4) : nullptr;
  if (nb && (!d_in || !d_desc || !d_status)) {
    undo();
    rfxi::set_error("rfx_text_append_bgzf: no device memory for the staging area");
    return RFX_E_NOMEM;
  }
  hipError_t rc = hipSuccess;
  if (nb) {  // (the spans: rfx_prof_* from ONE appending thread, as the measurement scripts do)
    rfx_span sp(c, "bgzf_copy", t->copy);
    rc = hipMemcpyAsync(d_in, host, n, hipMemcpyHostToDevice, t->copy);
    if (rc == hipSuccess) rc = hipMemcpyAsync(d_desc, ds.data(), (size_t)nb * sizeof(bgzf_desc), hipMemcpyHostToDevice, t->copy);
  }
  if (rc == hipSuccess) rc = hipEventRecord(t->ev[t->n_ev], t->copy);  // the host buffer is free
  if (rc == hipSuccess && nb) {
    rc = hipEventRecord(t->staged, t->copy);
    if (rc == hipSuccess) rc = hipStreamWaitEvent(t->kern, t->staged, 0);
    if (rc == hipSuccess) {
      rfx_span sp(c, "k_bgzf_inflate", t->kern);
      rfxk::bgzf_inflate(c, t->kern, d_in, d_desc, nb, t->n_bgzf_blocks, t->arena, d_status, t->first_bad);
      rc = hipGetLastError();
    }
  }
  if (rc != hipSuccess) {
    // (what was queued before the failing call may still read the staging bytes: they are handed out again only after
    // the streams have drained)
    (void)hipStreamSynchronize(t->copy);
    (void)hipStreamSynchronize(t->kern);
    undo();
    return hip_fail(rc, "rfx_text_append_bgzf");
  }
  if (nb) {
    t->bgzf.push_back({t->n_bgzf_blocks, nb, d_status});
    t->n_bgzf_blocks += nb;
  }
  t->used += inflated;
  return (long)t->n_ev++;
}

// rfx_text_settle (max_records = all of them) and rfx_text_settle_records: the cut lies behind newline number
// 4 * min(floor(N / 4), max_records); *records (may be null) = that minimum
static int settle_at(rfx_text* t, rfx_text* next, uint64_t max_records, uint64_t* records, uint64_t* carried, const char* who) {
  if (!t || !carried || next == t) return RFX_E_INVAL;
  *carried = 0;
  if (records) *records = 0;
  if (next && (next->used != 0 || next->ctx != t->ctx)) return RFX_E_INVAL;
  rfx_ctx* c = t->ctx;
  (void)hipSetDevice(c->device);
  HIPCHK(hipStreamSynchronize(t->copy));
  if (t->kern) HIPCHK(hipStreamSynchronize(t->kern));
  if (const int rc = bgzf_check(t)) return rc;
  const uint64_t n = t->used;
  if (n == 0) return RFX_OK;
  HIPCHK(hipMemsetAsync(t->arena + n, 0, 2 * TX_TILE, c->stream));  // whole tiles are read, as in rfx_text_parse
  const uint64_t n_tiles = (n + TX_TILE - 1) / TX_TILE;
  uint64_t* tile_off = (uint64_t*)dmalloc(c, (n_tiles + 2) * 8);  // [n_tiles + 1]: the cut
  if (!tile_off) return RFX_E_NOMEM;
  const int grid = (int)std::min<uint64_t>(n_tiles, (uint64_t)c->n_cu * 8);
  {
    rfx_span sp(c, "k_txt_count");
    hipLaunchKernelGGL(k_txt_count, dim3(grid), dim3(TX_BLOCK), 0, c->stream, (const uint4*)t->arena, n_tiles, tile_off);
  }
  rfxk::scan_tail(c, tile_off, n_tiles);
  uint64_t n_lines = 0, cut = 0;
  hipError_t e = queue_read(c, &n_lines, tile_off + n_tiles, 8);
  if (e == hipSuccess) e = ctx_sync(c);
  const uint64_t n_rec = std::min(n_lines / 4, max_records);
  const uint64_t want = 4 * n_rec;  // newline number 4 * floor(N / 4) ends the last whole record
  if (e == hipSuccess && want) {
    {
      rfx_span sp(c, "k_txt_nth");
      hipLaunchKernelGGL(k_txt_nth, dim3(1), dim3(TX_BLOCK), 0, c->stream, (const uint4*)t->arena, n_tiles, tile_off, want,
                         tile_off + n_tiles + 1);
    }
    e = queue_read(c, &cut, tile_off + n_tiles + 1, 8);
    if (e == hipSuccess) e = ctx_sync(c);
  }
  dfree(c, tile_off);
  if (e != hipSuccess) return hip_fail(e, who);
  if (cut > n) {
    rfxi::set_error((std::string(who) + ": the cut lies behind the text").c_str());
    return RFX_E_HIP;
  }
  if (const int rc = rfxi::text_cut(t, next, cut, carried, who)) return rc;
  if (records) *records = n_rec;
  return RFX_OK;
}

int rfx_text_settle(rfx_text* t, rfx_text* next, uint64_t* carried) {
  return settle_at(t, next, ~0ull, nullptr, carried, "rfx_text_settle");
}

int rfx_text_settle_records(rfx_text* t, rfx_text* next, uint64_t max_records, uint64_t* records, uint64_t* carried) {
  if (!records) return RFX_E_INVAL;
  return settle_at(t, next, max_records, records, carried, "rfx_text_settle_records");
}

int rfx_text_records(rfx_text* t, uint64_t* records) {
  if (!t || !records) return RFX_E_INVAL;
  *records = 0;
  rfx_ctx* c = nullptr;
  const uint8_t* arena = nullptr;
  uint64_t n = 0;
  if (const int rc = rfxi::text_ready(t, &c, &arena, &n)) return rc;
  if (n == 0) return RFX_OK;
  const uint64_t n_tiles = (n + TX_TILE - 1) / TX_TILE;
  uint64_t* tile_off = (uint64_t*)dmalloc(c, (n_tiles + 1) * 8);
  if (!tile_off) return RFX_E_NOMEM;
  uint64_t n_lines = 0;
  hipError_t e = rfxi::text_count_lines(c, arena, n, tile_off);
  if (e == hipSuccess) e = queue_read(c, &n_lines, tile_off + n_tiles, 8);
  const hipError_t es = ctx_sync(c);  // (also when queueing failed: nothing may still point at n_lines)
  dfree(c, tile_off);
  if (e != hipSuccess || es != hipSuccess) return hip_fail(e != hipSuccess ? e : es, "rfx_text_records");
  *records = n_lines / 4;
  return RFX_OK;
}

rfx_reads* rfx_text_parse(rfx_text* t, int flags, int min_q, int* strict) {
  if (strict) *strict = 1;
  if (!t || !strict || (flags != RFX_PACK_COUNT && flags != RFX_PACK_FILTER)) return nullptr;
  rfx_ctx* c = t->ctx;
  (void)hipSetDevice(c->device);
  const uint64_t n = t->used;
  auto not_strict = [&]() -> rfx_reads* {
    *strict = 0;
    return nullptr;
  };
  if (n == 0) return not_strict();
  if (bgzf_check(t) != RFX_OK) return nullptr;  // (an arena that never saw a BGZF append: nothing happens here)
  {  // the ctx stream waits for the copies (they ran on the arena's own stream)
    std::lock_guard<std::mutex> g(t->mu);
    if (t->n_ev && hipStreamWaitEvent(c->stream, t->ev[t->n_ev - 1], 0) != hipSuccess) return nullptr;
  }
  // (BGZF appends: bgzf_check above has waited for their kernels)
  // whole tiles are read: what lies behind the text holds no newline
  if (hipMemsetAsync(t->arena + n, 0, 2 * TX_TILE, c->stream) != hipSuccess) return nullptr;
  const uint64_t n_tiles = (n + TX_TILE - 1) / TX_TILE;
  uint64_t* tile_off = (uint64_t*)dmalloc(c, (n_tiles + 1) * 8);
  txt_stats* st = (txt_stats*)dmalloc(c, sizeof(txt_stats));
  uint32_t* line_start = nullptr;
  uint64_t* words = nullptr;
  rfx_reads* r = nullptr;
  auto drop = [&] { dfree(c, tile_off); dfree(c, st); dfree(c, line_start); dfree(c, words); };
  auto fail = [&](const char* what, hipError_t e) -> rfx_reads* {
    if (e != hipSuccess) hip_fail(e, what);
    (void)ctx_sync(c);  // (a read-back queued before the failure points at a local of this function: deliver it now)
    drop();
    if (r) rfx_reads_free(r);
    return nullptr;
  };
  if (!tile_off || !st) return fail("rfx_text_parse", hipSuccess);
  hipError_t e = hipMemsetAsync(st, 0, sizeof(txt_stats), c->stream);
  if (e != hipSuccess) return fail("rfx_text_parse", e);
  const int grid = (int)std::min<uint64_t>(n_tiles, (uint64_t)c->n_cu * 8);
  {
    rfx_span sp(c, "k_txt_count");
    hipLaunchKernelGGL(k_txt_count, dim3(grid), dim3(TX_BLOCK), 0, c->stream, (const uint4*)t->arena, n_tiles, tile_off);
  }
  rfxk::scan_tail(c, tile_off, n_tiles);
  uint64_t n_lines = 0;
  unsigned char last = 0;
  e = queue_read(c, &n_lines, tile_off + n_tiles, 8);
  if (e == hipSuccess) e = queue_read(c, &last, t->arena + n - 1, 1);
  if (e == hipSuccess) e = ctx_sync(c);
  if (e != hipSuccess) return fail("rfx_text_parse", e);
  // every line ends with its newline (the caller closes a file's last line), four lines per record
  if (last != '\n' || n_lines == 0 || (n_lines & 3u) || n_lines / 4 > 0xFFFFFFFEull) {
    drop();
    return not_strict();
  }
  const uint64_t n_reads = n_lines / 4;
  line_start = (uint32_t*)dmalloc(c, (n_lines + 1) * 4);
  words = (uint64_t*)dmalloc(c, (n_reads + 1) * 8);
  r = new rfx_reads();
  memset(r, 0, sizeof *r);
  r->gen = rfx_next_reads_gen();
  r->ctx = c;
  r->n = (uint32_t)n_reads;
  r->len = (uint32_t*)dmalloc(c, n_reads * 4);
  r->word_off = (uint32_t*)dmalloc(c, (n_reads + 1) * 4);
  if (!line_start || !words || !r->len || !r->word_off) return fail("rfx_text_parse", hipSuccess);
  e = hipMemsetAsync(line_start, 0, 4, c->stream);
  if (e != hipSuccess) return fail("rfx_text_parse", e);
  {
    rfx_span sp(c, "k_txt_lines");
    hipLaunchKernelGGL(k_txt_lines, dim3(grid), dim3(TX_BLOCK), 0, c->stream, (const uint4*)t->arena, n_tiles, tile_off, line_start,
                       n_lines);
  }
  {
    rfx_span sp(c, "k_txt_reads");
    hipLaunchKernelGGL(k_txt_reads, dim3((unsigned)std::min<uint64_t>((n_reads + 255) / 256, (uint64_t)c->n_cu * 16)), dim3(256), 0,
                       c->stream, t->arena, line_start, n_reads, r->len, words, st);
  }
  rfxk::scan_tail(c, words, n_reads);
  txt_stats hs;
  uint64_t n_words = 0;
  e = queue_read(c, &hs, st, sizeof hs);
  if (e == hipSuccess) e = queue_read(c, &n_words, words + n_reads, 8);
  if (e == hipSuccess) e = ctx_sync(c);
  if (e != hipSuccess) return fail("rfx_text_parse", e);
  if (hs.bad || n_words > 0xFFFFFFFFull) {
    drop();
    rfx_reads_free(r);
    return not_strict();
  }
  r->n_words = n_words;
  r->n_bases = hs.n_bases;
  r->max_len = hs.max_len;
  memcpy(r->short_cnt, hs.short_cnt, sizeof r->short_cnt);
  r->codes = (uint64_t*)dmalloc(c, std::max<uint64_t>(n_words, 1) * 8);
  uint32_t* mask = (uint32_t*)dmalloc(c, std::max<uint64_t>(n_words, 1) * 4);
  if (flags == RFX_PACK_COUNT) r->acgt = mask;
  else r->good = mask;
  if (!r->codes || !mask) return fail("rfx_text_parse", hipSuccess);
  const uint32_t maxw = std::max<uint32_t>(1, (hs.max_len + 31) / 32);
  const uint64_t total = n_reads * maxw;
  const unsigned pgrid = (unsigned)std::min<uint64_t>((total + 255) / 256, (uint64_t)c->n_cu * 32);
  {
    rfx_span sp(c, "k_txt_pack");
    if (flags == RFX_PACK_FILTER)
      hipLaunchKernelGGL(k_txt_pack<true>, dim3(pgrid), dim3(256), 0, c->stream, t->arena, line_start, words, r->len, n_reads, maxw,
                         min_q, r->codes, mask, r->word_off, st);
    else
      hipLaunchKernelGGL(k_txt_pack<false>, dim3(pgrid), dim3(256), 0, c->stream, t->arena, line_start, words, r->len, n_reads, maxw,
                         min_q, r->codes, mask, r->word_off, st);
  }
  // (the arena may be appended to again once this returns: the pack has read it)
  e = ctx_sync(c);
  drop();
  if (e != hipSuccess) {
    hip_fail(e, "rfx_text_parse");
    rfx_reads_free(r);
    return nullptr;
  }
  return r;
}

}  // extern "C"
