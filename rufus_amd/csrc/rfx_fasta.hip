// FASTA TEXT in a text arena -> a packed read block, and the cut of an arena at a FASTA record, on the device.
//
// Replaces, for a reference FASTA kept as `ref.fa.gz` (bgzip), the `zcat ref.fa.gz | jellyfish count ... /dev/stdin` in
// front of the -e / -f databases of runRufus.sh:77,115 and the contig / window counts of Overlap.shorter.sh:245,255: the
// parser of jf/include/jellyfish/mer_overlap_sequence_parser.hpp:124-251 on text that exists only in HBM (k_bgzf_inflate
// wrote it there, rfx_text_append_bgzf).  The rule is rfx_fasta_core.h, one source for host and device.
//
// rfx_text_parse_fasta:
//   k_txt_count / k_txt_lines (rfx_text.hip)   the line starts
//   k_fa_lines     a thread per line: fa_line_key (header count << 32 | sequence bytes) and a non-empty flag
//                                                         -> two scans: a line's record and first base; the compacted list
//   k_fa_scatter   a thread per line: a header writes its record's first base index, a non-empty sequence line its entry of
//                  the compacted list (first base index, first byte)
//   k_fa_reads     a thread per record: len, words; the longest read by a 32-bit atomicMax      -> scan -> word offsets
//   k_fa_pack      a thread per OUTPUT code word (fa_pack_word): read by binary search in the word offsets, line by binary
//                  search in the compacted list, at most 32 line steps and 32 bases; one store per code and mask word.
//                  (k_txt_pack walks reads x longest-read words: here one read is a chromosome.)
// rfx_text_settle_fasta:
//   k_fa_last_header   a thread per line start: a 32-bit atomicMax over those whose byte is '>'
//
// Bounds: every text index is compared with the arena's byte count before the load (rfx_fasta_core.h); every list index
// with the list's count.  The block is what rfx_pack_reads(RFX_PACK_COUNT) makes of the joined sequences, max_len
// included, so rfx_count_add's tiler (rfx_tile.hip) and every counting route take it unchanged.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <string>

#include "rfx_fasta_core.h"
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

constexpr uint64_t FA_TILE = 4096;  // rfx_text.hip's TX_TILE: the tile of k_txt_count's counts

struct fa_stats {
  unsigned int max_len;
  unsigned int short_cnt[32];
};

// line i = text[ls[i], e), e = ls[i + 1] - 1 (where its '\n' lies) or n for a last line without one
__global__ __launch_bounds__(256) void k_fa_lines(const uint8_t* __restrict__ text, uint64_t n, const uint32_t* __restrict__ ls,
                                                   uint64_t n_nl, uint64_t n_lines, uint64_t* __restrict__ key,
                                                   uint64_t* __restrict__ nonempty) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_lines; i += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t b = ls[i], e = i < n_nl ? (uint64_t)ls[i + 1] - 1u : n;
    const uint64_t k = fa_line_key(text, n, b, e);
    key[i] = k;
    nonempty[i] = fa_key_bases(k) ? 1u : 0u;
  }
}

// key / ne: the exclusive scans of k_fa_lines' arrays (entry n_lines = the totals)
__global__ __launch_bounds__(256) void k_fa_scatter(const uint32_t* __restrict__ ls, const uint64_t* __restrict__ key,
                                                     const uint64_t* __restrict__ ne, uint64_t n_lines, uint32_t n_rec, uint32_t n_ne,
                                                     uint32_t* __restrict__ rec_base, uint32_t* __restrict__ ne_base,
                                                     uint32_t* __restrict__ ne_src) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_lines; i += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t at = key[i], mine = key[i + 1] - at;
    if (i == 0) rec_base[n_rec] = ne_base[n_ne] = fa_key_bases(key[n_lines]);
    if (fa_key_headers(mine)) {
      const uint32_t r = fa_key_headers(at);
      if (r < n_rec) rec_base[r] = fa_key_bases(at);
    } else if (fa_key_bases(mine)) {
      const uint64_t q = ne[i];
      if (q < n_ne) {
        ne_base[q] = fa_key_bases(at);
        ne_src[q] = ls[i];
      }
    }
  }
}

__global__ __launch_bounds__(256) void k_fa_reads(const uint32_t* __restrict__ rec_base, uint32_t n_rec, uint32_t* __restrict__ len,
                                                   uint64_t* __restrict__ words, fa_stats* __restrict__ st) {
  for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n_rec; r += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t L = rec_base[r + 1] - rec_base[r];
    len[r] = L;
    words[r] = (L + 31u) / 32u;
    atomicMax(&st->max_len, L);
    if (L < 32u) atomicAdd(&st->short_cnt[L], 1u);
  }
}

// items [0, n_rec]: word_off; items [0, n_words): one code word and one mask word each
__global__ __launch_bounds__(256) void k_fa_pack(const uint8_t* __restrict__ text, uint64_t n, const uint64_t* __restrict__ word_off64,
                                                  const uint32_t* __restrict__ rec_base, uint32_t n_rec,
                                                  const uint32_t* __restrict__ ne_base, const uint32_t* __restrict__ ne_src, uint32_t n_ne,
                                                  uint64_t n_words, uint64_t* __restrict__ codes, uint32_t* __restrict__ mask,
                                                  uint32_t* __restrict__ word_off) {
  const uint64_t items = n_words > n_rec ? n_words : (uint64_t)n_rec + 1u;
  for (uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; w < items; w += (uint64_t)gridDim.x * blockDim.x) {
    if (w <= n_rec) word_off[w] = (uint32_t)word_off64[w];
    if (w >= n_words) continue;
    const uint32_t r = fa_last_le_u64(word_off64, n_rec, w);
    const uint64_t j = w - word_off64[r];
    const uint32_t first = rec_base[r], L = rec_base[r + 1] - first;
    uint64_t c = 0;
    uint32_t m = 0;
    if (j * 32u < L) {
      const uint32_t done = (uint32_t)j * 32u;
      fa_pack_word(text, n, ne_base, ne_src, n_ne, first + done, min(32u, L - done), &c, &m);
    }
    codes[w] = c;
    mask[w] = m;
  }
}

// *cut = the largest line start p = ls[i], 1 <= i <= n_nl, with p < n and text[p] == '>' (zeroed by the caller: none)
__global__ __launch_bounds__(256) void k_fa_last_header(const uint8_t* __restrict__ text, uint64_t n, const uint32_t* __restrict__ ls,
                                                         uint64_t n_nl, uint32_t* __restrict__ cut) {
  for (uint64_t i = 1 + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i <= n_nl; i += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t p = ls[i];
    if (fa_is_header(text, n, p, n)) atomicMax(cut, p);
  }
}

unsigned grid_for(rfx_ctx* c, uint64_t items, unsigned per_cu) {
  return (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((items + 255) / 256, (uint64_t)c->n_cu * per_cu));
}

// the line starts of arena[0, n) on the ctx stream: *n_nl newlines, ls[0 .. n_nl]; first / last = the text's end bytes.
// One wait.  The caller frees *ls.
int line_starts(rfx_ctx* c, const uint8_t* arena, uint64_t n, uint32_t** ls, uint64_t* n_nl, unsigned char* first,
                unsigned char* last, const char* who) {
  const uint64_t n_tiles = (n + FA_TILE - 1) / FA_TILE;
  uint64_t* tile_off = (uint64_t*)dmalloc(c, (n_tiles + 1) * 8);
  if (!tile_off) return RFX_E_NOMEM;
  hipError_t e = rfxi::text_count_lines(c, arena, n, tile_off);
  if (e == hipSuccess) e = queue_read(c, n_nl, tile_off + n_tiles, 8);
  if (e == hipSuccess) e = queue_read(c, first, arena, 1);
  if (e == hipSuccess) e = queue_read(c, last, arena + n - 1, 1);
  const hipError_t es = rfxi::sync(c);  // (also when queueing failed: nothing may still point at the caller's locals)
  if (e == hipSuccess) e = es;
  if (e == hipSuccess && *first == '>') {
    *ls = (uint32_t*)dmalloc(c, (*n_nl + 2) * 4);
    if (!*ls) {
      dfree(c, tile_off);
      return RFX_E_NOMEM;
    }
    e = rfxi::text_line_starts(c, arena, n, tile_off, *ls, *n_nl);
  }
  dfree(c, tile_off);  // stream-ordered
  return e == hipSuccess ? RFX_OK : hip_fail(e, who);
}

}  // namespace

extern "C" {

int rfx_text_settle_fasta(rfx_text* t, rfx_text* next, uint64_t* carried) {
  if (!t || !carried || next == t) return RFX_E_INVAL;
  *carried = 0;
  if (next && (rfx_text_bytes(next) != 0 || rfxi::text_ctx(next) != rfxi::text_ctx(t))) return RFX_E_INVAL;
  rfx_ctx* c = nullptr;
  const uint8_t* arena = nullptr;
  uint64_t n = 0;
  if (const int rc = rfxi::text_ready(t, &c, &arena, &n)) return rc;
  if (n == 0) return RFX_OK;
  uint32_t* ls = nullptr;
  uint64_t n_nl = 0;
  unsigned char first = 0, last = 0;
  if (const int rc = line_starts(c, arena, n, &ls, &n_nl, &first, &last, "rfx_text_settle_fasta")) return rc;
  if (first != '>') {
    rfxi::set_error("rfx_fasta: the text does not begin with '>'");
    return RFX_E_FORMAT;
  }
  uint64_t cut = n;  // next == NULL: the file ends here, and a last line without '\n' is a line
  if (next) {
    uint32_t* d_cut = (uint32_t*)dmalloc(c, 4);
    uint32_t h_cut = 0;
    hipError_t e = d_cut ? hipMemsetAsync(d_cut, 0, 4, c->stream) : hipErrorOutOfMemory;
    if (e == hipSuccess) {
      {
        rfx_span sp(c, "k_fa_last_header");
        hipLaunchKernelGGL(k_fa_last_header, dim3(grid_for(c, n_nl, 16)), dim3(256), 0, c->stream, arena, n, ls, n_nl, d_cut);
      }
      e = hipGetLastError();
    }
    if (e == hipSuccess) e = queue_read(c, &h_cut, d_cut, 4);
    const hipError_t es = rfxi::sync(c);
    dfree(c, d_cut);
    dfree(c, ls);
    if (e != hipSuccess || es != hipSuccess) return hip_fail(e != hipSuccess ? e : es, "rfx_text_settle_fasta");
    if (h_cut == 0 || h_cut >= n) {  // the arena's last record is carried: nothing says it is whole before the next header
      char msg[160];
      snprintf(msg, sizeof msg, "rfx_fasta: one sequence fills the text arena of %llu bytes", (unsigned long long)n);
      rfxi::set_error(msg);
      return RFX_E_RANGE;
    }
    cut = h_cut;
  } else {
    const hipError_t es = rfxi::sync(c);  // (k_txt_lines has read the arena)
    dfree(c, ls);
    if (es != hipSuccess) return hip_fail(es, "rfx_text_settle_fasta");
  }
  return rfxi::text_cut(t, next, cut, carried, "rfx_text_settle_fasta");
}

rfx_reads* rfx_text_parse_fasta(rfx_text* t, int flags, int* fasta) {
  if (fasta) *fasta = 1;
  if (!t || !fasta) {
    rfxi::set_error("rfx_text_parse_fasta: RFX_E_INVAL: a NULL argument");
    return nullptr;
  }
  if (flags != RFX_PACK_COUNT) {
    rfxi::set_error("rfx_text_parse_fasta: RFX_E_INVAL: FASTA has no qualities: RFX_PACK_COUNT only");
    return nullptr;
  }
  rfx_ctx* c = nullptr;
  const uint8_t* arena = nullptr;
  uint64_t n = 0;
  if (rfxi::text_ready(t, &c, &arena, &n) != RFX_OK) return nullptr;  // (a block that did not inflate: as rfx_text_parse)
  auto not_fasta = [&]() -> rfx_reads* {
    *fasta = 0;
    return nullptr;
  };
  if (n == 0) return not_fasta();
  uint32_t* ls = nullptr;
  uint64_t n_nl = 0;
  unsigned char first = 0, last = 0;
  if (line_starts(c, arena, n, &ls, &n_nl, &first, &last, "rfx_text_parse_fasta") != RFX_OK) return nullptr;
  if (first != '>') return not_fasta();
  const uint64_t n_lines = n_nl + (last != '\n' ? 1u : 0u);  // >= 1

  uint64_t *key = (uint64_t*)dmalloc(c, (n_lines + 1) * 8), *ne = (uint64_t*)dmalloc(c, (n_lines + 1) * 8), *words = nullptr;
  uint32_t *rec_base = nullptr, *ne_base = nullptr, *ne_src = nullptr;
  fa_stats* st = (fa_stats*)dmalloc(c, sizeof(fa_stats));
  rfx_reads* r = nullptr;
  auto drop = [&] {
    dfree(c, ls); dfree(c, key); dfree(c, ne); dfree(c, words); dfree(c, rec_base); dfree(c, ne_base); dfree(c, ne_src); dfree(c, st);
  };
  auto fail = [&](hipError_t e, const char* text) -> rfx_reads* {
    if (e != hipSuccess) hip_fail(e, "rfx_text_parse_fasta");
    else if (text) rfxi::set_error(text);
    (void)rfxi::sync(c);  // (a read-back queued before the failure points at a local of this function: deliver it now)
    drop();
    if (r) rfx_reads_free(r);
    return nullptr;
  };
  const char* nomem = "rfx_text_parse_fasta: RFX_E_NOMEM: no device memory for the block";
  if (!key || !ne || !st) return fail(hipSuccess, nomem);
  hipError_t e = hipMemsetAsync(st, 0, sizeof(fa_stats), c->stream);
  if (e != hipSuccess) return fail(e, nullptr);
  {
    rfx_span sp(c, "k_fa_lines");
    hipLaunchKernelGGL(k_fa_lines, dim3(grid_for(c, n_lines, 16)), dim3(256), 0, c->stream, arena, n, ls, n_nl, n_lines, key, ne);
  }
  rfxk::scan_tail(c, key, n_lines);
  rfxk::scan_tail(c, ne, n_lines);
  uint64_t key_all = 0, ne_all = 0;
  e = queue_read(c, &key_all, key + n_lines, 8);
  if (e == hipSuccess) e = queue_read(c, &ne_all, ne + n_lines, 8);
  if (e == hipSuccess) e = rfxi::sync(c);
  if (e != hipSuccess) return fail(e, nullptr);
  const uint64_t n_rec = key_all >> 32, n_bases = key_all & 0xFFFFFFFFull;
  if (n_rec == 0 || n_rec > 0xFFFFFFFEull || ne_all > 0xFFFFFFFEull)  // (the first line is a header: n_rec >= 1)
    return fail(hipSuccess, "rfx_text_parse_fasta: RFX_E_RANGE: 2^32 reads or more in one arena");
  const uint32_t n_ne = (uint32_t)ne_all;

  rec_base = (uint32_t*)dmalloc(c, (n_rec + 1) * 4);
  ne_base = (uint32_t*)dmalloc(c, ((uint64_t)n_ne + 1) * 4);
  ne_src = (uint32_t*)dmalloc(c, ((uint64_t)n_ne + 1) * 4);
  words = (uint64_t*)dmalloc(c, (n_rec + 1) * 8);
  r = new rfx_reads();
  memset(r, 0, sizeof *r);
  r->gen = rfx_next_reads_gen();
  r->ctx = c;
  r->n = (uint32_t)n_rec;
  r->len = (uint32_t*)dmalloc(c, n_rec * 4);
  r->word_off = (uint32_t*)dmalloc(c, (n_rec + 1) * 4);
  if (!rec_base || !ne_base || !ne_src || !words || !r->len || !r->word_off) return fail(hipSuccess, nomem);
  {
    rfx_span sp(c, "k_fa_scatter");
    hipLaunchKernelGGL(k_fa_scatter, dim3(grid_for(c, n_lines, 16)), dim3(256), 0, c->stream, ls, key, ne, n_lines, (uint32_t)n_rec,
                       n_ne, rec_base, ne_base, ne_src);
  }
  {
    rfx_span sp(c, "k_fa_reads");
    hipLaunchKernelGGL(k_fa_reads, dim3(grid_for(c, n_rec, 16)), dim3(256), 0, c->stream, rec_base, (uint32_t)n_rec, r->len, words, st);
  }
  rfxk::scan_tail(c, words, n_rec);
  fa_stats hs;
  uint64_t n_words = 0;
  e = queue_read(c, &hs, st, sizeof hs);
  if (e == hipSuccess) e = queue_read(c, &n_words, words + n_rec, 8);
  if (e == hipSuccess) e = rfxi::sync(c);
  if (e != hipSuccess) return fail(e, nullptr);
  if (n_words > 0xFFFFFFFFull) return fail(hipSuccess, "rfx_text_parse_fasta: RFX_E_RANGE: 2^32 code words or more in one arena");
  r->n_words = n_words;
  r->n_bases = n_bases;
  r->max_len = hs.max_len;
  memcpy(r->short_cnt, hs.short_cnt, sizeof r->short_cnt);
  r->codes = (uint64_t*)dmalloc(c, std::max<uint64_t>(n_words, 1) * 8);
  r->acgt = (uint32_t*)dmalloc(c, std::max<uint64_t>(n_words, 1) * 4);
  if (!r->codes || !r->acgt) return fail(hipSuccess, nomem);
  {
    rfx_span sp(c, "k_fa_pack");
    hipLaunchKernelGGL(k_fa_pack, dim3(grid_for(c, std::max<uint64_t>(n_words, n_rec + 1), 32)), dim3(256), 0, c->stream, arena, n,
                       words, rec_base, (uint32_t)n_rec, ne_base, ne_src, n_ne, n_words, r->codes, r->acgt, r->word_off);
  }
  // (the arena may be appended to again once this returns: the pack has read it)
  e = rfxi::sync(c);
  if (e != hipSuccess) return fail(e, nullptr);
  drop();
  return r;
}

}  // extern "C"
