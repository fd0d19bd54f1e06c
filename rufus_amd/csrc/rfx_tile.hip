// Long sequences -> a block of reads of at most `tile_len` bases with the same k-mer windows, on the device.
//
// Every count kernel gives one lane to one read, which suits reads of 76 .. 250 bases and not a FASTA of chromosomes or
// contigs (the reference walks those with the same loop as reads: jf/include/jellyfish/mer_overlap_sequence_parser.hpp:
// 124-251 hands the sequence out in overlapping buffers, mer_iterator.hpp:59-88 slides over them).  A window that starts
// at base p of a sequence lies in exactly one tile when the tiles are tile_len bases long and start every
// step = tile_len - k + 1 bases: tile p / step.  So the tiled block has the k-mer multiset of the source, masks included,
// and is an ordinary block to every count path (whole-read kernels, run maps, shard passes).
//
//   k_reads_tile_count   tiles and output words of every read                                   -> two scans
//   k_reads_tile_table   one thread per tile: len[], word_off[] of the tiled block
//   k_reads_tile   one thread per OUTPUT word: the two source code words and the two source mask words it spans,
//                  funnel-shifted by the tile's start; bits beyond the tile's length are 0 (as rfx_pack_reads leaves them)
//
// The shifts are lane-varying; they stay in 32-bit halves (v_alignbit_b32), no 64-bit shift by a lane's own amount.
#include <algorithm>
#include <cstdio>
#include <cstring>

#include "rfx_internal.h"

using rfxi::dfree;
using rfxi::dmalloc;
using rfxi::queue_read;

extern "C" int rfx_tile_plan(uint64_t len, int k, uint32_t tile_len, uint64_t* n_tiles, uint32_t* step) {
  if (k < 1 || k > 32 || tile_len < (uint32_t)k) return RFX_E_INVAL;
  const uint32_t st = tile_len - (uint32_t)k + 1u;
  if (step) *step = st;
  if (n_tiles) *n_tiles = len <= tile_len ? 1 : (len - (uint64_t)k + 1 + st - 1) / st;
  return RFX_OK;
}

namespace {

__device__ __forceinline__ uint32_t tiles_of(uint32_t len, uint32_t k, uint32_t L, uint32_t step) {
  return len <= L ? 1u : (uint32_t)(((uint64_t)len - k + step) / step);  // ceil((len - k + 1) / step)
}

// tiles[r] / words[r]: tiles and output words of read r; d_short[l] += last tiles of multi-tile reads that are l < 32
// bases long (the one-tile reads are counted by the source block already)
__global__ __launch_bounds__(256) void k_reads_tile_count(rfx_reads_view rv, uint32_t k, uint32_t L, uint32_t step, uint32_t wpt,
                                                     uint64_t* __restrict__ tiles, uint64_t* __restrict__ words,
                                                     unsigned int* __restrict__ d_short) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < rv.n; i += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t r = (uint32_t)i;
    const uint32_t len = rv_len(rv, r);
    const uint32_t nt = tiles_of(len, k, L, step);
    const uint32_t last = len - (nt - 1u) * step;
    tiles[r] = nt;
    words[r] = (uint64_t)(nt - 1u) * wpt + (last + 31u) / 32u;
    if (nt > 1u && last < 32u) atomicAdd(&d_short[last], 1u);
  }
}

// the last i in [0, n) with off[i] <= x (off is non-decreasing, off[0] = 0 <= x)
__device__ __forceinline__ uint32_t owner_of(const uint64_t* __restrict__ off, uint32_t n, uint64_t x) {
  uint32_t lo = 0, hi = n;
  while (hi - lo > 1u) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (off[mid] <= x) lo = mid;
    else hi = mid;
  }
  return lo;
}

__global__ __launch_bounds__(256) void k_reads_tile_table(rfx_reads_view rv, uint32_t L, uint32_t step, uint32_t wpt,
                                                     const uint64_t* __restrict__ tile_off, const uint64_t* __restrict__ word_base,
                                                     uint64_t n_tiles, uint32_t* __restrict__ out_len,
                                                     uint32_t* __restrict__ out_word_off) {
  for (uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; g < n_tiles; g += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t r = owner_of(tile_off, rv.n, g);
    const uint32_t t = (uint32_t)(g - tile_off[r]);
    const uint32_t rest = rv_len(rv, r) - t * step;
    out_len[g] = min(L, rest);
    out_word_off[g] = (uint32_t)(word_base[r] + (uint64_t)t * wpt);
    if (g == 0) out_word_off[n_tiles] = (uint32_t)word_base[rv.n];
  }
}

__device__ __forceinline__ uint32_t low_bits(uint32_t n) { return n >= 32u ? ~0u : (1u << n) - 1u; }  // n ones

__global__ __launch_bounds__(256) void k_reads_tile(rfx_reads_view rv, uint32_t L, uint32_t step, uint32_t wpt,
                                                     const uint64_t* __restrict__ word_base, uint64_t n_words,
                                                     uint2* __restrict__ out_codes, uint32_t* __restrict__ out_mask) {
  for (uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; w < n_words; w += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t r = owner_of(word_base, rv.n, w);
    const uint32_t wi = (uint32_t)(w - word_base[r]);
    const uint32_t t = wi / wpt, j = wi - t * wpt;       // (a one-tile read has fewer than wpt words: t = 0)
    const uint32_t len = rv_len(rv, r);
    const uint32_t tlen = min(L, len - t * step);
    const uint32_t nb = min(32u, tlen - j * 32u);        // bases of this word: 1 .. 32
    const uint32_t p = t * step + j * 32u;               // its first base in the read
    const uint32_t sw = p >> 5, sh = p & 31u;
    const bool two = sh + nb > 32u;                      // the bases run on into the next source word (it exists then)
    const uint32_t soff = rv_off(rv, r);
    const uint2* src = (const uint2*)(rv.codes + soff + sw);
    const uint2 a = src[0];
    const uint2 b = two ? src[1] : make_uint2(0u, 0u);
    // 128 bits a.x a.y b.x b.y shifted right by 2 * sh (0 .. 62) bits, in 32-bit halves
    const uint32_t bs = (2u * sh) & 31u;
    const bool hi = sh >= 16u;
    const uint32_t w0 = hi ? a.y : a.x, w1 = hi ? b.x : a.y, w2 = hi ? b.y : b.x;
    uint32_t c0 = __funnelshift_r(w0, w1, bs), c1 = __funnelshift_r(w1, w2, bs);
    c0 &= low_bits(2u * nb);
    c1 &= nb > 16u ? low_bits(2u * nb - 32u) : 0u;
    const uint32_t* am = rv_acgt(rv, r, soff);
    uint32_t m = ~0u;
    if (am) m = __funnelshift_r(am[sw], two ? am[sw + 1] : 0u, sh);
    out_codes[w] = make_uint2(c0, c1);
    out_mask[w] = m & low_bits(nb);
  }
}

}  // namespace

namespace rfxi {

rfx_reads* reads_tile(rfx_ctx* c, const rfx_reads* src, int k, uint32_t tile_len, int* rc_out) {
  int rc_local;
  int& rc = rc_out ? *rc_out : rc_local;
  rc = RFX_E_INVAL;
  uint32_t step = 0;
  if (!c || !src || src->ctx != c || (!src->acgt && !src->ulen) || rfx_tile_plan(0, k, tile_len, nullptr, &step) != RFX_OK) {
    set_error("rfx_reads_tile: needs a count block (ACGT mask) of this context, 1 <= k <= 32 and tile_len >= k");
    return nullptr;
  }
  (void)hipSetDevice(c->device);
  const uint32_t n = src->n;
  const uint32_t wpt = (tile_len + 31u) / 32u;
  // (an upper bound from what the host knows refuses the hopeless cases before anything is allocated)
  if ((src->n_bases / step + n) >= (1ull << 32)) {
    rc = RFX_E_RANGE;
    set_error("rfx_reads_tile: RFX_E_RANGE: the tiled block would reach 2^32 tiles");
    return nullptr;
  }
  rfx_reads* r = new rfx_reads();
  memset(r, 0, sizeof *r);
  r->gen = rfx_next_reads_gen();
  r->ctx = c;
  uint64_t* tile_off = (uint64_t*)dmalloc(c, ((size_t)n + 1) * 8);
  uint64_t* word_base = (uint64_t*)dmalloc(c, ((size_t)n + 1) * 8);
  unsigned int* d_short = (unsigned int*)dmalloc(c, 32 * 4);
  auto fail = [&](int code, hipError_t e, const char* text) -> rfx_reads* {
    rc = code;
    if (e != hipSuccess) {
      char msg[256];
      snprintf(msg, sizeof msg, "rfx_reads_tile: %s", hipGetErrorString(e));
      set_error(msg);
    } else if (text) {
      set_error(text);
    }
    (void)rfxi::sync(c);  // (a queued read-back points at a local of this function: deliver it now)
    dfree(c, tile_off); dfree(c, word_base); dfree(c, d_short);
    rfx_reads_free(r);
    return nullptr;
  };
  if (!tile_off || !word_base || !d_short) return fail(RFX_E_NOMEM, hipSuccess, "rfx_reads_tile: out of device memory");
  const rfx_reads_view rv = src->view();
  uint64_t totals[2] = {0, 0};  // tiles, words
  unsigned int h_short[32];
  memset(h_short, 0, sizeof h_short);
  if (n) {
    hipError_t e = hipMemsetAsync(d_short, 0, 32 * 4, c->stream);
    if (e != hipSuccess) return fail(RFX_E_HIP, e, nullptr);
    {
      rfx_span sp(c, "k_reads_tile_count");
      hipLaunchKernelGGL(k_reads_tile_count, dim3(std::min<uint32_t>((n + 255u) / 256u, (uint32_t)c->n_cu * 16u)), dim3(256), 0, c->stream, rv,
                         (uint32_t)k, tile_len, step, wpt, tile_off, word_base, d_short);
    }
    rfxk::scan_tail(c, tile_off, n);
    rfxk::scan_tail(c, word_base, n);
    e = queue_read(c, &totals[0], tile_off + n, 8);
    if (e == hipSuccess) e = queue_read(c, &totals[1], word_base + n, 8);
    if (e == hipSuccess) e = queue_read(c, h_short, d_short, sizeof h_short);
    if (e == hipSuccess) e = rfxi::sync(c);
    if (e != hipSuccess) return fail(RFX_E_HIP, e, nullptr);
  }
  const uint64_t T = totals[0], W = totals[1];
  if (T >= (1ull << 32) || W >= (1ull << 32))
    return fail(RFX_E_RANGE, hipSuccess, "rfx_reads_tile: RFX_E_RANGE: the tiled block would reach 2^32 tiles or words");
  r->n = (uint32_t)T;
  r->n_words = W;
  r->n_bases = src->n_bases + (uint64_t)(k - 1) * (T - n);  // neighbouring tiles share k - 1 bases
  r->max_len = std::min(src->max_len, tile_len);
  for (int l = 0; l < 32; ++l) r->short_cnt[l] = src->short_cnt[l] + h_short[l];
  r->codes = (uint64_t*)dmalloc(c, std::max<uint64_t>(W, 1) * 8);
  r->acgt = (uint32_t*)dmalloc(c, std::max<uint64_t>(W, 1) * 4);
  r->word_off = (uint32_t*)dmalloc(c, ((size_t)T + 1) * 4);
  r->len = (uint32_t*)dmalloc(c, std::max<uint64_t>(T, 1) * 4);
  if (!r->codes || !r->acgt || !r->word_off || !r->len) return fail(RFX_E_NOMEM, hipSuccess, "rfx_reads_tile: out of device memory");
  hipError_t e = hipSuccess;
  if (T == 0) {
    e = hipMemsetAsync(r->word_off, 0, 4, c->stream);
  } else {
    {
      rfx_span sp(c, "k_reads_tile_table");
      hipLaunchKernelGGL(k_reads_tile_table, dim3((unsigned)std::min<uint64_t>((T + 255) / 256, (uint64_t)c->n_cu * 16)), dim3(256), 0, c->stream,
                         rv, tile_len, step, wpt, tile_off, word_base, T, r->len, r->word_off);
    }
    if (W) {
      rfx_span sp(c, "k_reads_tile");
      hipLaunchKernelGGL(k_reads_tile, dim3((unsigned)std::min<uint64_t>((W + 255) / 256, (uint64_t)c->n_cu * 32)), dim3(256), 0, c->stream,
                         rv, tile_len, step, wpt, word_base, W, (uint2*)r->codes, r->acgt);
    }
  }
  if (e == hipSuccess) e = rfxi::sync(c);
  if (e != hipSuccess) return fail(RFX_E_HIP, e, nullptr);
  dfree(c, tile_off); dfree(c, word_base); dfree(c, d_short);
  rc = RFX_OK;
  return r;
}

}  // namespace rfxi

extern "C" rfx_reads* rfx_reads_tile(rfx_ctx* c, const rfx_reads* src, int k, uint32_t tile_len) {
  return rfxi::reads_tile(c, src, k, tile_len, nullptr);
}
