// Reads of one or several blocks, chosen by per-read bit masks that lie on the device -> ONE new dense block, in source
// order.  What the reference does in the write loop of src/RUFUS.Filter.cpp after :196-277 -- "a pair is written when either
// mate reached the threshold" -- for reads that exist only as packed blocks in HBM.
//
// A read starts on a word boundary in every block, so a selected read's words are copied as they are: the result is what
// rfx_pack_reads would make of the selected reads' text, whatever flags the source was packed with.
//
//   k_select_words   one thread per mask word (64 reads): the effective word (pair rule, bits >= n cleared), its selected
//                    reads, their code words and bases                                          -> three scans
//                    (+ the longest selected read and the histogram of lengths < 32: atomics on 33 counters)
//   k_select_table   one thread per mask word: len[], word_off[] and the origin of its selected reads, at word base + rank
//   k_select_copy    one thread per OUTPUT word: owner by binary search in word_off, source word = rv_off(source read) + j;
//                    8 B of codes, 4 B of good, 4 B of mask (a compact read without a mask entry: ones up to its length)
//
// The effective word is computed twice (it is three instructions) instead of stored.  The loops over a word's set bits work
// on its 32-bit halves: no 64-bit shift by a lane's own amount in this file (rv_acgt's, which every kernel shares, aside).
#include <algorithm>
#include <cstdio>
#include <cstring>

#include "rfx_internal.h"

using rfxi::dfree;
using rfxi::dmalloc;
using rfxi::queue_read;

namespace {

constexpr uint64_t EVEN = 0x5555555555555555ull;

// bits of mask word w (of a block of n reads) that select a read; `tail` = the valid bits of the block's last word
__device__ __forceinline__ uint64_t effective_word(const uint64_t* __restrict__ mask, uint32_t w, uint32_t nw, uint64_t tail,
                                                   int pairs) {
  uint64_t m = mask[w];
  if (w == nw - 1u) m &= tail;  // (the filter kernels do not promise zeros there, and bit n must not pull read n - 1)
  if (pairs) {
    m |= ((m & EVEN) << 1) | ((m >> 1) & EVEN);  // mates 2p and 2p + 1 share a word
    if (w == nw - 1u) m &= tail;                 // (the last read of an odd block has no mate)
  }
  return m;
}

__global__ __launch_bounds__(256) void k_select_words(rfx_reads_view rv, const uint64_t* __restrict__ mask, uint32_t nw, uint64_t tail,
                                                      int pairs, uint64_t* __restrict__ cnt, uint64_t* __restrict__ words,
                                                      uint64_t* __restrict__ bases, unsigned int* __restrict__ d_stat) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nw; i += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t w = (uint32_t)i;
    const uint64_t m = effective_word(mask, w, nw, tail, pairs);
    const uint32_t c = (uint32_t)__popcll(m);
    uint64_t nwords = 0, nbases = 0;
    uint32_t longest = 0;
    if (rv.ulen) {  // compact: every read alike
      nwords = (uint64_t)c * rv.uwpr;
      nbases = (uint64_t)c * rv.ulen;
      longest = c ? rv.ulen : 0u;
      if (c && rv.ulen < 32u) atomicAdd(&d_stat[1u + rv.ulen], c);
    } else {
      for (uint32_t h = 0; h < 2u; ++h) {
        uint32_t bits = h ? (uint32_t)(m >> 32) : (uint32_t)m;
        while (bits) {
          const uint32_t b = (uint32_t)__ffs(bits) - 1u;
          bits &= bits - 1u;
          const uint32_t len = rv.len[w * 64u + h * 32u + b];
          nwords += (len + 31u) / 32u;
          nbases += len;
          longest = max(longest, len);
          if (len < 32u) atomicAdd(&d_stat[1u + len], 1u);
        }
      }
    }
    cnt[w] = c;
    words[w] = nwords;
    bases[w] = nbases;
    if (longest) atomicMax(&d_stat[0], longest);
  }
}

// cnt / words: the scanned arrays, offset to this block's first mask word (so their values are positions in the result)
__global__ __launch_bounds__(256) void k_select_table(rfx_reads_view rv, const uint64_t* __restrict__ mask, uint32_t nw, uint64_t tail,
                                                      int pairs, uint32_t block, const uint64_t* __restrict__ cnt,
                                                      const uint64_t* __restrict__ words, uint32_t* __restrict__ out_len,
                                                      uint32_t* __restrict__ out_word_off, uint32_t* __restrict__ org_block,
                                                      uint32_t* __restrict__ org_read) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nw; i += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t w = (uint32_t)i;
    const uint64_t m = effective_word(mask, w, nw, tail, pairs);
    uint32_t o = (uint32_t)cnt[w], at = (uint32_t)words[w];  // (both totals are below 2^32: checked before this launch)
    for (uint32_t h = 0; h < 2u; ++h) {
      uint32_t bits = h ? (uint32_t)(m >> 32) : (uint32_t)m;
      while (bits) {
        const uint32_t b = (uint32_t)__ffs(bits) - 1u;
        bits &= bits - 1u;
        const uint32_t r = w * 64u + h * 32u + b;
        const uint32_t len = rv_len(rv, r);
        out_len[o] = len;
        out_word_off[o] = at;
        org_block[o] = block;
        org_read[o] = r;
        ++o;
        at += (len + 31u) / 32u;
      }
    }
  }
}

// the last i in [0, n) with off[i] <= x (off is non-decreasing, off[0] = 0 <= x)
__device__ __forceinline__ uint32_t owner_of(const uint32_t* __restrict__ off, uint32_t n, uint32_t x) {
  uint32_t lo = 0, hi = n;
  while (hi - lo > 1u) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (off[mid] <= x) lo = mid;
    else hi = mid;
  }
  return lo;
}

__device__ __forceinline__ uint32_t low_bits(uint32_t n) { return n >= 32u ? ~0u : (1u << n) - 1u; }  // n ones

__global__ __launch_bounds__(256) void k_select_copy(const rfx_reads_view* __restrict__ views, const uint32_t* __restrict__ word_off,
                                                     const uint32_t* __restrict__ org_block, const uint32_t* __restrict__ org_read,
                                                     uint32_t n_sel, uint64_t n_words, uint2* __restrict__ out_codes,
                                                     uint32_t* __restrict__ out_acgt, uint32_t* __restrict__ out_good) {
  for (uint64_t x = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; x < n_words; x += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t o = owner_of(word_off, n_sel, (uint32_t)x);
    const uint32_t j = (uint32_t)x - word_off[o];
    const rfx_reads_view& rv = views[org_block[o]];
    const uint32_t r = org_read[o];
    const uint32_t soff = rv_off(rv, r);
    out_codes[x] = ((const uint2*)rv.codes)[(size_t)soff + j];
    if (out_good) out_good[x] = rv.good[(size_t)soff + j];
    if (out_acgt) {  // (asked for only when every source block has a mask)
      const uint32_t* am = rv_acgt(rv, r, soff);
      out_acgt[x] = am ? am[j] : low_bits(rv_len(rv, r) - j * 32u);
    }
  }
}

}  // namespace

namespace rfxi {

rfx_reads* reads_select_dev(rfx_ctx* c, const rfx_reads* const* blocks, const uint64_t* const* d_masks, int n_blocks, int mode,
                            const char* who) {
  char msg[256];
  // (callers have checked the blocks, their context and the mode)
  (void)hipSetDevice(c->device);
  std::vector<uint64_t> wbase((size_t)n_blocks + 1, 0);  // first mask word of every block in the call's word space
  bool want_good = n_blocks > 0, want_acgt = n_blocks > 0;
  for (int i = 0; i < n_blocks; ++i) {
    wbase[(size_t)i + 1] = wbase[(size_t)i] + ((uint64_t)blocks[i]->n + 63) / 64;
    want_good = want_good && blocks[i]->good;
    want_acgt = want_acgt && (blocks[i]->acgt || blocks[i]->ulen);
  }
  const uint64_t MW = wbase[(size_t)n_blocks];
  rfx_reads* r = new rfx_reads();
  memset(r, 0, sizeof *r);
  r->gen = rfx_next_reads_gen();
  r->ctx = c;
  uint64_t* cnt = (uint64_t*)dmalloc(c, (MW + 1) * 8);
  uint64_t* words = (uint64_t*)dmalloc(c, (MW + 1) * 8);
  uint64_t* bases = (uint64_t*)dmalloc(c, (MW + 1) * 8);
  unsigned int* d_stat = (unsigned int*)dmalloc(c, 33 * 4);  // [0] longest selected read, [1 + l] selected reads of l < 32 bases
  rfx_reads_view* d_views = (rfx_reads_view*)dmalloc(c, std::max(n_blocks, 1) * sizeof(rfx_reads_view));
  auto fail = [&](hipError_t e, const char* code, const char* text) -> rfx_reads* {
    snprintf(msg, sizeof msg, "%s: %s%s%s", who, code, *code ? ": " : "", e != hipSuccess ? hipGetErrorString(e) : text);
    (void)rfxi::sync(c);  // (queued read-backs point at locals of this function: deliver them now)
    set_error(msg);
    dfree(c, cnt); dfree(c, words); dfree(c, bases); dfree(c, d_stat); dfree(c, d_views);
    rfx_reads_free(r);
    return nullptr;
  };
  if (!cnt || !words || !bases || !d_stat || !d_views) return fail(hipSuccess, "RFX_E_NOMEM", "out of device memory");
  uint64_t totals[3] = {0, 0, 0};  // reads, words, bases
  unsigned int h_stat[33];
  memset(h_stat, 0, sizeof h_stat);
  std::vector<rfx_reads_view> views((size_t)std::max(n_blocks, 1));
  for (int i = 0; i < n_blocks; ++i) views[(size_t)i] = blocks[i]->view();
  auto grid_of = [&](uint64_t n, int per_cu) { return dim3((unsigned)std::min<uint64_t>((n + 255) / 256, (uint64_t)c->n_cu * per_cu)); };
  auto tail_of = [](uint32_t n) { return (n & 63u) ? (1ull << (n & 63u)) - 1ull : ~0ull; };
  if (MW) {
    hipError_t e = hipMemsetAsync(d_stat, 0, 33 * 4, c->stream);
    if (e != hipSuccess) return fail(e, "RFX_E_HIP", "");
    for (int i = 0; i < n_blocks; ++i) {
      const uint32_t nw = (uint32_t)(wbase[(size_t)i + 1] - wbase[(size_t)i]);
      if (!nw) continue;
      rfx_span sp(c, "k_select_words");
      hipLaunchKernelGGL(k_select_words, grid_of(nw, 16), dim3(256), 0, c->stream, views[(size_t)i], d_masks[i], nw,
                         tail_of(blocks[i]->n), mode == RFX_SELECT_PAIRS, cnt + wbase[(size_t)i], words + wbase[(size_t)i],
                         bases + wbase[(size_t)i], d_stat);
    }
    rfxk::scan_tail(c, cnt, MW);
    rfxk::scan_tail(c, words, MW);
    rfxk::scan_tail(c, bases, MW);
    e = queue_read(c, &totals[0], cnt + MW, 8);
    if (e == hipSuccess) e = queue_read(c, &totals[1], words + MW, 8);
    if (e == hipSuccess) e = queue_read(c, &totals[2], bases + MW, 8);
    if (e == hipSuccess) e = queue_read(c, h_stat, d_stat, sizeof h_stat);
    if (e == hipSuccess) e = hipMemcpyAsync(d_views, views.data(), (size_t)n_blocks * sizeof(rfx_reads_view), hipMemcpyHostToDevice, c->stream);
    if (e != hipSuccess) return fail(e, "RFX_E_HIP", "");
  }
  // the first wait: the totals the result is allocated by (and whatever the caller queued before: the filter's counts and masks)
  {
    const hipError_t e = rfxi::sync(c);
    if (e != hipSuccess) return fail(e, "RFX_E_HIP", "");
  }
  const uint64_t S = totals[0], W = totals[1];
  if (S >= (1ull << 32) || W >= (1ull << 32)) return fail(hipSuccess, "RFX_E_RANGE", "the selection would reach 2^32 reads or words");
  r->n = (uint32_t)S;
  r->n_words = W;
  r->n_bases = totals[2];
  r->max_len = h_stat[0];
  for (int l = 0; l < 32; ++l) r->short_cnt[l] = h_stat[1 + l];
  r->codes = (uint64_t*)dmalloc(c, std::max<uint64_t>(W, 1) * 8);
  if (want_acgt) r->acgt = (uint32_t*)dmalloc(c, std::max<uint64_t>(W, 1) * 4);
  if (want_good) r->good = (uint32_t*)dmalloc(c, std::max<uint64_t>(W, 1) * 4);
  r->word_off = (uint32_t*)dmalloc(c, ((size_t)S + 1) * 4);
  r->len = (uint32_t*)dmalloc(c, std::max<uint64_t>(S, 1) * 4);
  r->org_block = (uint32_t*)dmalloc(c, std::max<uint64_t>(S, 1) * 4);
  r->org_read = (uint32_t*)dmalloc(c, std::max<uint64_t>(S, 1) * 4);
  r->has_origin = 1;
  if (!r->codes || (want_acgt && !r->acgt) || (want_good && !r->good) || !r->word_off || !r->len || !r->org_block || !r->org_read)
    return fail(hipSuccess, "RFX_E_NOMEM", "out of device memory");
  const uint32_t w_end = (uint32_t)W;
  hipError_t e = hipSuccess;
  if (S == 0) {
    e = hipMemsetAsync(r->word_off, 0, 4, c->stream);
  } else {
    e = hipMemcpyAsync(r->word_off + S, &w_end, 4, hipMemcpyHostToDevice, c->stream);  // (w_end lives until the wait below)
    for (int i = 0; i < n_blocks && e == hipSuccess; ++i) {
      const uint32_t nw = (uint32_t)(wbase[(size_t)i + 1] - wbase[(size_t)i]);
      if (!nw) continue;
      rfx_span sp(c, "k_select_table");
      hipLaunchKernelGGL(k_select_table, grid_of(nw, 16), dim3(256), 0, c->stream, views[(size_t)i], d_masks[i], nw,
                         tail_of(blocks[i]->n), mode == RFX_SELECT_PAIRS, (uint32_t)i, cnt + wbase[(size_t)i],
                         words + wbase[(size_t)i], r->len, r->word_off, r->org_block, r->org_read);
    }
    if (W && e == hipSuccess) {
      rfx_span sp(c, "k_select_copy");
      hipLaunchKernelGGL(k_select_copy, grid_of(W, 32), dim3(256), 0, c->stream, d_views, r->word_off, r->org_block, r->org_read,
                         (uint32_t)S, W, (uint2*)r->codes, r->acgt, r->good);
    }
  }
  if (e == hipSuccess) e = rfxi::sync(c);  // the second wait
  if (e != hipSuccess) return fail(e, "RFX_E_HIP", "");
  dfree(c, cnt); dfree(c, words); dfree(c, bases); dfree(c, d_stat); dfree(c, d_views);
  return r;
}

}  // namespace rfxi

extern "C" int rfx_reads_origin(const rfx_reads* r, uint32_t* block_out, uint32_t* read_out) {
  if (!r || !r->has_origin) return RFX_E_INVAL;
  rfx_ctx* c = r->ctx;
  (void)hipSetDevice(c->device);
  hipError_t e = hipSuccess;
  if (r->n && block_out) e = hipMemcpyAsync(block_out, r->org_block, (size_t)r->n * 4, hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess && r->n && read_out) e = hipMemcpyAsync(read_out, r->org_read, (size_t)r->n * 4, hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = rfxi::sync(c);
  if (e != hipSuccess) {
    char msg[256];
    snprintf(msg, sizeof msg, "rfx_reads_origin: %s", hipGetErrorString(e));
    rfxi::set_error(msg);
    return RFX_E_HIP;
  }
  return RFX_OK;
}
