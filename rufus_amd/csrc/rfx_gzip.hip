// Plain gzip inflated on the device (rfx_text_append_gzip): a deflate stream without BGZF's framing has no independent
// pieces, so they are made -- found speculatively, sized by a walk, confirmed on the host by the chain rule of
// rfx_gzip_core.h (gz_append), decoded with an unknown 32 KiB history into 16-bit values and then repaired.  Replaces the
// inflate of `zcat F.fastq.gz | ...` (runRufus.sh:157-160, :229-232, :974-977).
//
//   k_gz_find     a wave per nominal boundary: 4 x 64 bit offsets at a time through gz_prefilter (registers only), the
//                 survivors of each ballot through gz_probe on the wave's bgzf_tables in LDS, lowest first; the first that
//                 passes is the boundary's candidate.  The search ends at the next boundary.
//   k_gz_walk     a wave per chunk, from its start to the next chunk's start: gz_run with nothing stored
//                 -> (end_bit, out_bytes, final, status)
//   k_gz_inflate  a wave per confirmed chunk: gz_run into the 16-bit side buffer at the offset the walk's sizes give; the
//                 lanes spread literal runs, matches and stored runs as k_bgzf_inflate's do
//   k_gz_windows  ONE workgroup, chunks in order: each chunk's last 32 KiB of 16-bit values resolved into the arena
//                 against the 32 KiB in front of the chunk (the stream's window buffer for what lies before the batch);
//                 leaves the batch's last 32 KiB in the other window buffer.  The only serial step.
//   k_gz_resolve  a thread per four output bytes, all chunks at once: every value resolved through its chunk's window,
//                 which is final by then.  (It stores the windows' bytes a second time, with the values they hold.)
//   k_gz_crc      a wave per 64 KiB of a chunk's bytes: lane slices, each shifted to the chunk's end, XORed into the
//                 chunk's word -- bgzf_crc_update(0, chunk): the host combines them in order against the trailer.
//
// One wave per workgroup wherever rfx_gzip_core.h's statements run (lockstep: see rfx_bgzf.hip); LDS: one bgzf_tables,
// 4160 bytes.  Bounds: the core reads input inside [stage, stage + n) only; a chunk's wave writes side[out_off,
// out_off + out_bytes) only (max_out is the walk's size); the host checks used + total <= cap before the launches.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "rfx_gzip_core.h"
#include "rfx_internal.h"

namespace {

struct gz_dchunk {
  uint64_t start, stop;         // bits of the staged input
  uint64_t out_off, out_bytes;  // in the batch (k_gz_inflate and behind)
  uint32_t first, pad;
};
constexpr uint32_t GZ_CRC_SEG = 65536;
constexpr uint32_t GZ_FIND_ROWS = 4;

__global__ __launch_bounds__(64) void k_gz_find(const uint8_t* __restrict__ stage, uint64_t n, uint64_t first_boundary,
                                                 uint32_t chunk_bytes, uint32_t n_bound, uint64_t* __restrict__ cand) {
  __shared__ bgzf_tables tables;
  const uint32_t lane = threadIdx.x;
  const uint8_t* end = stage + n;
  for (uint32_t k = blockIdx.x; k < n_bound; k += gridDim.x) {
    const uint64_t lo_bit = (first_boundary + (uint64_t)k * chunk_bytes) * 8u;
    const uint64_t hi_bit = min(lo_bit + (uint64_t)chunk_bytes * 8u, n * 8u);
    uint64_t found = ~0ull;
    for (uint64_t base = lo_bit; base < hi_bit && found == ~0ull; base += 64u * GZ_FIND_ROWS) {
      bool pass[GZ_FIND_ROWS];  // GZ_FIND_ROWS x 64 bit offsets per turn: their loads are in flight together
#pragma unroll
      for (uint32_t j = 0; j < GZ_FIND_ROWS; ++j) {
        const uint64_t bit = base + 64u * j + lane;
        uint64_t lo = 0, hi = 0;
        if (bit < hi_bit) gz_bits128(stage, end, bit, &lo, &hi);
        pass[j] = bit < hi_bit && gz_prefilter(lo, hi);
      }
#pragma unroll
      for (uint32_t j = 0; j < GZ_FIND_ROWS; ++j) {
        uint64_t m = __ballot(pass[j]);
        while (m && found == ~0ull) {  // (wave-uniform) lowest bit offset first
          const uint32_t l = (uint32_t)__ffsll((unsigned long long)m) - 1u;
          m &= m - 1u;
          if (gz_probe(stage, end, base + 64u * j + l, tables)) found = base + 64u * j + l;
        }
      }
    }
    if (lane == 0) cand[k] = found;
  }
}

__global__ __launch_bounds__(64) void k_gz_walk(const uint8_t* __restrict__ stage, uint64_t n, const gz_dchunk* __restrict__ ch,
                                                 uint32_t n_ch, gz_result* __restrict__ res) {
  __shared__ bgzf_tables tables;
  for (uint32_t c = blockIdx.x; c < n_ch; c += gridDim.x) {
    const gz_dchunk d = ch[c];
    gz_null_out no;
    gz_result r;
    gz_run(stage, stage + n, d.start, d.stop, d.first != 0u, ~0ull, tables, no, r);
    __syncthreads();  // the tables are free for the next chunk
    if (threadIdx.x == 0) res[c] = r;
  }
}

// The 16-bit policy of rfx_gzip_core.h (gz_serial16), spread over the wave; ordering as rfx_bgzf.hip's wave_out.
struct wave_out16 {
  uint16_t* out;
  uint32_t lane;
  uint32_t n_lit, lit;
  uint64_t lit_pos;
  int64_t synced;  // every store to out[0, synced) is visible to all lanes

  __device__ __forceinline__ void flush() {
    if (lane < n_lit) out[lit_pos + lane] = (uint16_t)lit;
    n_lit = 0;
  }
  __device__ __forceinline__ void literal(uint64_t pos, uint32_t byte) {
    if (n_lit == 0) lit_pos = pos;
    if (lane == n_lit) lit = byte;
    if (++n_lit == 64u) flush();
  }
  __device__ __forceinline__ void match(uint64_t pos, uint32_t len, uint32_t dist) {
    flush();
    const int64_t src = (int64_t)pos - (int64_t)dist, src_end = src + (int64_t)(len < dist ? len : dist);
    if (src_end > synced) {  // (wave-uniform: every lane of the one-wave workgroup arrives)
      __syncthreads();
      synced = (int64_t)pos;
    }
    for (uint32_t i = lane; i < len; i += 64u) {
      const int64_t j = src + (int64_t)(i < dist ? i : i % dist);
      // (dist <= GZ_WINDOW, so GZ_WINDOW + j >= 0: a marker names a byte of the 32 KiB in front of the chunk)
      out[pos + i] = j < 0 ? (uint16_t)(0x8000u | (uint32_t)((int64_t)GZ_WINDOW + j)) : out[j];
    }
  }
  __device__ __forceinline__ void stored(uint64_t pos, const uint8_t* from, uint32_t n) {
    flush();
    for (uint32_t i = lane; i < n; i += 64u) out[pos + i] = from[i];
  }
  __device__ __forceinline__ void end() { flush(); }
};

__global__ __launch_bounds__(64) void k_gz_inflate(const uint8_t* __restrict__ stage, uint64_t n, const gz_dchunk* __restrict__ ch,
                                                    uint32_t n_ch, uint16_t* side, gz_result* __restrict__ res) {
  __shared__ bgzf_tables tables;
  for (uint32_t c = blockIdx.x; c < n_ch; c += gridDim.x) {
    const gz_dchunk d = ch[c];
    wave_out16 wo{side + d.out_off, threadIdx.x, 0u, 0u, 0ull, 0};
    gz_result r;
    gz_run(stage, stage + n, d.start, d.stop, d.first != 0u, d.out_bytes, tables, wo, r);
    __syncthreads();
    if (threadIdx.x == 0) res[c] = r;
  }
}

constexpr int GZ_WIN_BLOCK = 1024, GZ_WIN_PER = GZ_WINDOW / GZ_WIN_BLOCK;
// gz_resolve16 with both loads unconditional (a value that is a byte reads win[0] and out[0] and drops them), so that a
// thread's GZ_WIN_PER values are in flight together: the chunks are taken one after the other, and a chunk costs the
// latency of its loads.
__device__ __forceinline__ uint32_t gz_resolve16_flat(uint32_t v, const uint8_t* out, const uint8_t* __restrict__ win, uint64_t off) {
  const bool marker = v >= 0x8000u;
  const uint64_t k = marker ? off + (v & 0x7FFFu) : 0u;  // index into win ++ out, as gz_history
  const uint32_t a = win[k < GZ_WINDOW ? k : 0u], b = out[k < GZ_WINDOW ? 0u : k - GZ_WINDOW];
  return !marker ? v : k < GZ_WINDOW ? a : b;
}

__global__ __launch_bounds__(GZ_WIN_BLOCK) void k_gz_windows(const uint16_t* __restrict__ side, const gz_dchunk* __restrict__ ch,
                                                              uint32_t n_ch, uint64_t total, uint8_t* out,
                                                              const uint8_t* __restrict__ win, uint8_t* __restrict__ win_next) {
  uint64_t off = ch[0].out_off, nb = ch[0].out_bytes;
  for (uint32_t c = 0; c < n_ch; ++c) {
    const uint64_t off_next = c + 1u < n_ch ? ch[c + 1u].out_off : 0u, nb_next = c + 1u < n_ch ? ch[c + 1u].out_bytes : 0u;
    const uint64_t k0 = (nb > GZ_WINDOW ? nb - GZ_WINDOW : 0u) + threadIdx.x;
    uint32_t v[GZ_WIN_PER];
#pragma unroll
    for (int i = 0; i < GZ_WIN_PER; ++i) {
      const uint64_t k = k0 + (uint64_t)i * GZ_WIN_BLOCK;
      v[i] = k < nb ? side[off + k] : 0u;
    }
#pragma unroll
    for (int i = 0; i < GZ_WIN_PER; ++i) v[i] = gz_resolve16_flat(v[i], out, win, off);  // (reads bytes in front of `off` only)
#pragma unroll
    for (int i = 0; i < GZ_WIN_PER; ++i) {
      const uint64_t k = k0 + (uint64_t)i * GZ_WIN_BLOCK;
      if (k < nb) out[off + k] = (uint8_t)v[i];
    }
    __syncthreads();  // the next chunk's window is this chunk's bytes
    off = off_next;
    nb = nb_next;
  }
  for (uint32_t k = threadIdx.x; k < GZ_WINDOW; k += GZ_WIN_BLOCK) {
    const uint64_t idx = total + k;  // the last 32 KiB of win ++ out
    win_next[k] = idx < GZ_WINDOW ? win[idx] : out[idx - GZ_WINDOW];
  }
}

__global__ __launch_bounds__(256) void k_gz_resolve(const uint16_t* __restrict__ side, const gz_dchunk* __restrict__ ch,
                                                     uint32_t n_ch, uint64_t total, uint8_t* out, const uint8_t* __restrict__ win) {
  const bool aligned = ((uintptr_t)out & 3u) == 0;
  for (uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; q * 4u < total; q += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t p0 = q * 4u;
    uint32_t lo = 0, hi = n_ch;  // the last chunk with out_off <= p0 (empty chunks share an offset with the one behind)
    while (hi - lo > 1u) {
      const uint32_t mid = (lo + hi) / 2u;
      if (ch[mid].out_off <= p0) lo = mid;
      else hi = mid;
    }
    uint32_t c = lo;
    uint64_t off = ch[c].out_off, cend = off + ch[c].out_bytes;
    uint32_t word = 0;
    const uint32_t nb = (uint32_t)min((uint64_t)4, total - p0);
    for (uint32_t i = 0; i < nb; ++i) {
      const uint64_t p = p0 + i;
      while (p >= cend) {  // (p < total: a chunk that holds it follows)
        ++c;
        off = ch[c].out_off;
        cend = off + ch[c].out_bytes;
      }
      word |= (uint32_t)gz_resolve16(side[p], out, win, off) << (8u * i);
    }
    if (aligned && nb == 4u) {
      *(uint32_t*)(out + p0) = word;
    } else {
      for (uint32_t i = 0; i < nb; ++i) out[p0 + i] = (uint8_t)(word >> (8u * i));
    }
  }
}

__global__ __launch_bounds__(64) void k_gz_crc(const uint8_t* __restrict__ out, const gz_dchunk* __restrict__ ch,
                                                const uint2* __restrict__ work, uint32_t n_work, uint32_t* crc) {
  const uint32_t lane = threadIdx.x;
  for (uint32_t w = blockIdx.x; w < n_work; w += gridDim.x) {
    const uint2 wk = work[w];
    const gz_dchunk d = ch[wk.x];
    const uint64_t seg_lo = (uint64_t)wk.y * GZ_CRC_SEG;
    const uint32_t len = (uint32_t)min((uint64_t)GZ_CRC_SEG, d.out_bytes - seg_lo);
    const uint32_t slice = (len + 63u) / 64u;
    const uint32_t lo = lane * slice < len ? lane * slice : len;
    const uint32_t hi = lo + slice < len ? lo + slice : len;
    uint32_t x = bgzf_crc_update(0u, out + d.out_off + seg_lo + lo, hi - lo);
    x = bgzf_crc_shift(x, (uint32_t)(d.out_bytes - seg_lo - hi));  // (a chunk fits an arena: < 4 GiB)
#pragma unroll
    for (int o = 32; o; o >>= 1) x ^= __shfl_xor(x, o);
    if (lane == 0) atomicXor(&crc[wk.x], x);
  }
}

int hip_fail(hipError_t e, const char* what) {
  char msg[256];
  snprintf(msg, sizeof msg, "%s: %s", what, hipGetErrorString(e));
  rfxi::set_error(msg);
  return RFX_E_HIP;
}
#define HIPCHK(x)                                   \
  do {                                              \
    hipError_t e_ = (x);                            \
    if (e_ != hipSuccess) return hip_fail(e_, #x);  \
  } while (0)

struct dbuf {  // a device buffer that only grows
  void* p = nullptr;
  size_t cap = 0;
  int want(size_t bytes) {
    if (bytes <= cap) return RFX_OK;
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
    const size_t c = std::max(bytes + bytes / 4, (size_t)4096);
    if (hipMalloc(&p, c) != hipSuccess) {
      (void)hipGetLastError();
      p = nullptr;
      rfxi::set_error("rfx_text_append_gzip: no device memory");
      return RFX_E_NOMEM;
    }
    cap = c;
    return RFX_OK;
  }
  void drop() {
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
  }
};

}  // namespace

struct rfx_gzip {
  rfx_ctx* ctx = nullptr;
  gz_stream S;
  dbuf stage, side, cand, chunks, res, crc, work;
  uint8_t* win[2] = {nullptr, nullptr};  // the stream's last 32 KiB: win[cur]; k_gz_windows writes the other
  int cur = 0;
};

namespace {

struct dev_backend {
  rfx_gzip* g;
  rfx_text* t;
  rfx_ctx* c;
  const uint8_t* host;
  uint64_t n;
  uint8_t* arena;
  uint64_t cap_, used;
  bool staged = false;

  uint64_t room() const { return cap_ - used; }
  uint64_t cap() const { return cap_; }
  int grid(uint64_t items) const { return (int)std::max<uint64_t>(1, std::min<uint64_t>(items, (uint64_t)c->n_cu * 32u * 16u)); }

  int stage_in() {
    if (staged) return RFX_OK;
    if (const int rc = g->stage.want((size_t)n + 16)) return rc;
    rfx_span sp(c, "gz_copy");
    HIPCHK(hipMemcpyAsync(g->stage.p, host, n, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemsetAsync((uint8_t*)g->stage.p + n, 0, 16, c->stream));
    staged = true;
    return RFX_OK;
  }
  int put_chunks(const std::vector<gz_dchunk>& d) {
    if (const int rc = g->chunks.want(d.size() * sizeof(gz_dchunk))) return rc;
    if (const int rc = g->res.want(d.size() * sizeof(gz_result))) return rc;
    HIPCHK(hipMemcpyAsync(g->chunks.p, d.data(), d.size() * sizeof(gz_dchunk), hipMemcpyHostToDevice, c->stream));
    return RFX_OK;
  }

  int find(uint64_t first_boundary, uint32_t chunk_bytes, std::vector<uint64_t>& out) {
    if (first_boundary >= n) return RFX_OK;
    if (const int rc = stage_in()) return rc;
    const uint64_t nb64 = (n - first_boundary + chunk_bytes - 1) / chunk_bytes;
    if (nb64 > 0x7FFFFFFFull) return RFX_E_RANGE;
    const uint32_t nb = (uint32_t)nb64;
    if (const int rc = g->cand.want((size_t)nb * 8)) return rc;
    {
      rfx_span sp(c, "k_gz_find");
      hipLaunchKernelGGL(k_gz_find, dim3(grid(nb)), dim3(64), 0, c->stream, (const uint8_t*)g->stage.p, n, first_boundary, chunk_bytes,
                         nb, (uint64_t*)g->cand.p);
    }
    HIPCHK(hipGetLastError());
    std::vector<uint64_t> all(nb);
    HIPCHK(hipMemcpyAsync(all.data(), g->cand.p, (size_t)nb * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(rfxi::sync(c));
    for (uint64_t b : all)
      if (b != ~0ull && b < n * 8u) out.push_back(b);
    return RFX_OK;
  }

  int walk(std::vector<gz_chunk>& list, const std::vector<uint32_t>& which) {
    if (const int rc = stage_in()) return rc;
    std::vector<gz_dchunk> d(which.size());
    for (size_t i = 0; i < which.size(); ++i) {
      const gz_chunk& k = list[which[i]];
      d[i] = gz_dchunk{k.start, k.stop, 0, 0, k.first, 0};
    }
    if (const int rc = put_chunks(d)) return rc;
    {
      rfx_span sp(c, "k_gz_walk");
      hipLaunchKernelGGL(k_gz_walk, dim3(grid(d.size())), dim3(64), 0, c->stream, (const uint8_t*)g->stage.p, n,
                         (const gz_dchunk*)g->chunks.p, (uint32_t)d.size(), (gz_result*)g->res.p);
    }
    HIPCHK(hipGetLastError());
    std::vector<gz_result> r(d.size());
    HIPCHK(hipMemcpyAsync(r.data(), g->res.p, r.size() * sizeof(gz_result), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(rfxi::sync(c));
    for (size_t i = 0; i < which.size(); ++i) list[which[i]].res = r[i];
    return RFX_OK;
  }

  int inflate(const gz_chunk* k, size_t nk, uint64_t total, uint32_t* crc_reg) {
    if (total > room()) return RFX_E_RANGE;
    if (total == 0) return RFX_OK;  // (empty members: nothing to store, every register 0)
    if (const int rc = stage_in()) return rc;
    std::vector<gz_dchunk> d(nk);
    std::vector<uint2> work;
    uint64_t off = 0;
    for (size_t i = 0; i < nk; ++i) {
      d[i] = gz_dchunk{k[i].start, k[i].stop, off, k[i].res.out_bytes, k[i].first, 0};
      for (uint64_t s = 0; s * GZ_CRC_SEG < k[i].res.out_bytes; ++s) work.push_back(make_uint2((uint32_t)i, (uint32_t)s));
      off += k[i].res.out_bytes;
    }
    if (const int rc = put_chunks(d)) return rc;
    if (const int rc = g->side.want(((size_t)total + 8) * 2)) return rc;
    if (const int rc = g->crc.want(nk * 4)) return rc;
    if (const int rc = g->work.want(work.size() * sizeof(uint2))) return rc;
    HIPCHK(hipMemcpyAsync(g->work.p, work.data(), work.size() * sizeof(uint2), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemsetAsync(g->crc.p, 0, nk * 4, c->stream));
    const gz_dchunk* dch = (const gz_dchunk*)g->chunks.p;
    uint8_t* out = arena + used;
    {
      rfx_span sp(c, "k_gz_inflate");
      hipLaunchKernelGGL(k_gz_inflate, dim3(grid(nk)), dim3(64), 0, c->stream, (const uint8_t*)g->stage.p, n, dch, (uint32_t)nk,
                         (uint16_t*)g->side.p, (gz_result*)g->res.p);
    }
    {
      rfx_span sp(c, "k_gz_windows");
      hipLaunchKernelGGL(k_gz_windows, dim3(1), dim3(GZ_WIN_BLOCK), 0, c->stream, (const uint16_t*)g->side.p, dch, (uint32_t)nk, total,
                         out, (const uint8_t*)g->win[g->cur], g->win[g->cur ^ 1]);
    }
    {
      rfx_span sp(c, "k_gz_resolve");
      hipLaunchKernelGGL(k_gz_resolve, dim3(grid((total / 4 + 255) / 256)), dim3(256), 0, c->stream, (const uint16_t*)g->side.p, dch,
                         (uint32_t)nk, total, out, (const uint8_t*)g->win[g->cur]);
    }
    {
      rfx_span sp(c, "k_gz_crc");
      hipLaunchKernelGGL(k_gz_crc, dim3(grid(work.size())), dim3(64), 0, c->stream, (const uint8_t*)out, dch,
                         (const uint2*)g->work.p, (uint32_t)work.size(), (uint32_t*)g->crc.p);
    }
    HIPCHK(hipGetLastError());
    std::vector<gz_result> r(nk);
    HIPCHK(hipMemcpyAsync(r.data(), g->res.p, nk * sizeof(gz_result), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(crc_reg, g->crc.p, nk * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(rfxi::sync(c));
    for (size_t i = 0; i < nk; ++i)  // the second decode of the same bits: anything else is a fault of this code
      if (r[i].status != BGZF_OK || r[i].out_bytes != k[i].res.out_bytes || r[i].end_bit != k[i].res.end_bit) {
        rfxi::set_error("rfx_text_append_gzip: the inflate of a chunk does not repeat its walk");
        return RFX_E_HIP;
      }
    g->cur ^= 1;
    used += total;
    rfxi::text_grow(t, total);
    return RFX_OK;
  }
};

}  // namespace

extern "C" {

rfx_gzip* rfx_gzip_open(rfx_ctx* c) {
  if (!c) return nullptr;
  (void)hipSetDevice(c->device);
  rfx_gzip* g = new rfx_gzip();
  g->ctx = c;
  g->S.e_format = RFX_E_FORMAT;
  if (const char* ev = getenv("RFX_GZIP_CHUNK")) {  // compressed bytes between two nominal boundaries: a power of two >= 1 KiB
    const long long v = atoll(ev);
    uint32_t cb = 1024;
    while (cb < (1u << 30) && (long long)cb * 2 <= v) cb *= 2;
    g->S.chunk_bytes = cb;
  }
  for (uint8_t*& w : g->win)
    if (hipMalloc((void**)&w, GZ_WINDOW) != hipSuccess || hipMemset(w, 0, GZ_WINDOW) != hipSuccess) {
      (void)hipGetLastError();
      rfx_gzip_close(g);
      return nullptr;
    }
  return g;
}

void rfx_gzip_close(rfx_gzip* g) {
  if (!g) return;
  (void)hipSetDevice(g->ctx->device);
  (void)rfxi::sync(g->ctx);
  for (dbuf* b : {&g->stage, &g->side, &g->cand, &g->chunks, &g->res, &g->crc, &g->work}) b->drop();
  for (uint8_t* w : g->win)
    if (w) (void)hipFree(w);
  delete g;
}

long rfx_text_append_gzip(rfx_text* t, rfx_gzip* g, const void* host, uint64_t n, int eof, uint64_t* consumed) {
  if (!t || !g || !consumed || (!host && n)) return RFX_E_INVAL;
  *consumed = 0;
  dev_backend B{g, t, nullptr, (const uint8_t*)host, n, nullptr, 0, 0};
  if (const int rc = rfxi::text_claim(t, &B.c, &B.arena, &B.cap_, &B.used)) return rc;
  if (B.c != g->ctx) return RFX_E_INVAL;
  const long rc = gz_append(g->S, B, (const uint8_t*)host, n, eof != 0, consumed);
  if (rc == RFX_E_FORMAT && !g->S.msg.empty()) rfxi::set_error(g->S.msg.c_str());
  return rc;
}

int rfx_gzip_stats(const rfx_gzip* g, uint64_t out[8]) {
  if (!g || !out) return RFX_E_INVAL;
  for (int i = 0; i < 8; ++i) out[i] = g->S.stats[i];
  return RFX_OK;
}

uint64_t rfx_gzip_need(const rfx_gzip* g) { return g ? g->S.need : 0; }

long rfx_gzip_starts(const rfx_gzip* g, uint64_t* out, uint64_t cap) {
  if (!g) return RFX_E_INVAL;
  for (uint64_t i = 0; out && i < cap && i < g->S.starts.size(); ++i) out[i] = g->S.starts[i];
  return (long)g->S.starts.size();
}

}  // extern "C"
