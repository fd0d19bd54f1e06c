// The TEXT of the records chosen by a per-record bit mask, gathered where it lies: the arena of rfx_text.hip -> one dense
// run of bytes on the host, in source order.  The text-side twin of rfx_select.hip: what the write loop of
// src/RUFUS.Filter.cpp after :196-277 does with the lines it still holds ("a pair is written when either mate reached the
// threshold"), for records whose text exists only in HBM (bgzip'd mates inflated on the device, runRufus.sh:977).
//
// A record is four lines, whatever they hold: record r is the arena's bytes [line_start[4r], line_start[4r + 4]).
//
//   k_txt_count / k_txt_lines   (rfx_text.hip) the arena's newlines and the byte behind each: recomputed here, so the call
//                               works with or without an rfx_text_parse before it
//   k_gather_sizes   one thread per mask word (64 records): its selected records and their bytes      -> two scans
//   k_gather_table   one thread per mask word: source offset and destination offset of its selected records, at rank
//   k_gather_copy    one thread per OUTPUT dword: owner by binary search in the destination offsets; the source dword is
//                    two aligned dword loads and a byte-align, whatever the source's residue against the destination's; a
//                    dword that straddles two records is put together from both; the last 1 - 3 bytes go by byte stores
//
// No LDS, no atomics: the output is a pure function of the arena and the mask.  The loops over a word's set bits work on
// its 32-bit halves (no 64-bit shift by a lane's own amount).  The arena is < 4 GiB: every offset is 32 bits.
#include <algorithm>
#include <cstdio>
#include <cstring>

#include "rfx_internal.h"

using rfxi::dfree;
using rfxi::dmalloc;
using rfxi::queue_read;

namespace {

__global__ __launch_bounds__(256) void k_gather_sizes(const uint32_t* __restrict__ line_start, const uint64_t* __restrict__ mask,
                                                      uint32_t nw, uint64_t tail, uint64_t* __restrict__ cnt,
                                                      uint64_t* __restrict__ bytes) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nw; i += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t w = (uint32_t)i;
    uint64_t m = mask[w];
    if (w == nw - 1u) m &= tail;  // bits at and above the record count are ignored
    uint64_t nbytes = 0;
    for (uint32_t h = 0; h < 2u; ++h) {
      uint32_t bits = h ? (uint32_t)(m >> 32) : (uint32_t)m;
      while (bits) {
        const uint32_t b = (uint32_t)__ffs(bits) - 1u;
        bits &= bits - 1u;
        const uint32_t r = w * 64u + h * 32u + b;
        nbytes += line_start[4u * r + 4u] - line_start[4u * r];
      }
    }
    cnt[w] = (uint32_t)__popcll(m);
    bytes[w] = nbytes;
  }
}

// cnt / bytes: the scanned arrays (positions in the result)
__global__ __launch_bounds__(256) void k_gather_table(const uint32_t* __restrict__ line_start, const uint64_t* __restrict__ mask,
                                                      uint32_t nw, uint64_t tail, const uint64_t* __restrict__ cnt,
                                                      const uint64_t* __restrict__ bytes, uint32_t* __restrict__ src_off,
                                                      uint32_t* __restrict__ dst_off) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nw; i += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t w = (uint32_t)i;
    uint64_t m = mask[w];
    if (w == nw - 1u) m &= tail;
    uint32_t o = (uint32_t)cnt[w], at = (uint32_t)bytes[w];  // (both totals are below 2^32: the arena is)
    for (uint32_t h = 0; h < 2u; ++h) {
      uint32_t bits = h ? (uint32_t)(m >> 32) : (uint32_t)m;
      while (bits) {
        const uint32_t b = (uint32_t)__ffs(bits) - 1u;
        bits &= bits - 1u;
        const uint32_t r = w * 64u + h * 32u + b;
        const uint32_t s = line_start[4u * r];
        src_off[o] = s;
        dst_off[o] = at;
        ++o;
        at += line_start[4u * r + 4u] - s;
      }
    }
    if (w == nw - 1u) dst_off[o] = at;  // dst_off[n_sel] = all bytes
  }
}

// the last i in [0, n) with off[i] <= x (off is increasing, off[0] = 0 <= x)
__device__ __forceinline__ uint32_t owner_of(const uint32_t* __restrict__ off, uint32_t n, uint32_t x) {
  uint32_t lo = 0, hi = n;
  while (hi - lo > 1u) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (off[mid] <= x) lo = mid;
    else hi = mid;
  }
  return lo;
}

// the four arena bytes from byte offset s on (any residue): two aligned dwords and a byte-align.  Reads up to 7 bytes
// behind s: the arena has 8 KiB of padding behind its capacity.
__device__ __forceinline__ uint32_t load_unaligned(const uint32_t* __restrict__ text, uint32_t s) {
  const uint32_t a = s >> 2;
  return __builtin_amdgcn_alignbyte(text[a + 1u], text[a], s & 3u);
}

// n_bytes > 0, n_sel > 0.  Thread x < n_bytes / 4 stores output dword x; thread n_bytes / 4 the last n_bytes % 4 bytes.
__global__ __launch_bounds__(256) void k_gather_copy(const uint32_t* __restrict__ text, const uint32_t* __restrict__ src_off,
                                                     const uint32_t* __restrict__ dst_off, uint32_t n_sel, uint32_t n_bytes,
                                                     uint32_t* __restrict__ out) {
  const uint32_t full = n_bytes >> 2;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i <= full; i += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t x = (uint32_t)i, d = x * 4u;
    if (d >= n_bytes) break;  // (n_bytes a multiple of four: no tail)
    const uint32_t o = owner_of(dst_off, n_sel, d);
    const uint32_t d0 = dst_off[o], end = dst_off[o + 1u];
    uint32_t v = load_unaligned(text, src_off[o] + (d - d0));
    const uint32_t have = end - d;  // bytes of this dword that record o holds (>= 1)
    if (have < 4u && o + 1u < n_sel) {
      // the rest is the beginning of record o + 1, which is at least four bytes long (four newlines): as if that record
      // had begun `have` bytes earlier (it is not the arena's first record: its source offset is >= 4 > have)
      const uint32_t v2 = load_unaligned(text, src_off[o + 1u] - have);
      const uint32_t keep = (1u << (8u * have)) - 1u;
      v = (v & keep) | (v2 & ~keep);
    }
    if (x < full) {
      out[x] = v;
    } else {  // the last 1 - 3 bytes of the output (all of record n_sel - 1, or put together as above)
      uint8_t* ob = (uint8_t*)out + d;
      for (uint32_t j = 0; j < n_bytes - d; ++j) ob[j] = (uint8_t)(v >> (8u * j));
    }
  }
}

int hip_fail(hipError_t e) {
  char msg[256];
  snprintf(msg, sizeof msg, "rfx_text_gather: %s", hipGetErrorString(e));
  rfxi::set_error(msg);
  return RFX_E_HIP;
}

}  // namespace

// k_gather_copy for another owner of the tables (rfx_bam_gather: a BAM record is at least 36 bytes, so what the kernel
// asks of a record -- four bytes or more, and not the arena's first where it follows another -- holds)
void rfxi::gather_copy(rfx_ctx* c, const uint8_t* arena, const uint32_t* src_off, const uint32_t* dst_off, uint32_t n_sel,
                       uint32_t n_bytes, uint32_t* out) {
  rfx_span sp(c, "k_gather_copy");
  const dim3 grid((unsigned)std::min<uint64_t>(((uint64_t)n_bytes / 4 + 1 + 255) / 256, (uint64_t)c->n_cu * 32));
  hipLaunchKernelGGL(k_gather_copy, grid, dim3(256), 0, c->stream, (const uint32_t*)arena, src_off, dst_off, n_sel, n_bytes, out);
}

extern "C" int rfx_text_gather(rfx_text* t, const uint64_t* hitmask, uint64_t n_records, void* host_out, uint64_t cap,
                               uint64_t* bytes_out, uint64_t* n_selected) {
  if (bytes_out) *bytes_out = 0;
  if (n_selected) *n_selected = 0;
  if (!t || !bytes_out || (n_records && !hitmask) || (cap && !host_out)) return RFX_E_INVAL;
  rfx_ctx* c = nullptr;
  const uint8_t* arena = nullptr;
  uint64_t n = 0;
  if (const int rc = rfxi::text_ready(t, &c, &arena, &n)) return rc;
  auto inval = [&] {
    rfxi::set_error("rfx_text_gather: the arena does not hold exactly n_records whole records");
    return RFX_E_INVAL;
  };
  // four newlines per record: n_records > n / 4 cannot be (and 4 * n_records + 1 line starts stay 32-bit indices)
  if (n_records > n / 4 || (n_records == 0) != (n == 0)) return inval();
  if (n == 0) return RFX_OK;
  const uint64_t n_tiles = (n + 4095) / 4096;
  const uint32_t nw = (uint32_t)((n_records + 63) / 64);
  const uint64_t tail = (n_records & 63u) ? (1ull << (n_records & 63u)) - 1ull : ~0ull;
  const uint64_t n_lines_want = 4 * n_records;
  uint64_t* tile_off = (uint64_t*)dmalloc(c, (n_tiles + 1) * 8);
  uint32_t* line_start = (uint32_t*)dmalloc(c, (n_lines_want + 1) * 4);
  uint64_t* d_mask = (uint64_t*)dmalloc(c, (size_t)nw * 8);
  uint64_t* cnt = (uint64_t*)dmalloc(c, ((size_t)nw + 1) * 8);
  uint64_t* sizes = (uint64_t*)dmalloc(c, ((size_t)nw + 1) * 8);
  uint32_t *src_off = nullptr, *dst_off = nullptr, *out = nullptr;
  auto drop = [&] {
    dfree(c, tile_off); dfree(c, line_start); dfree(c, d_mask); dfree(c, cnt); dfree(c, sizes);
    dfree(c, src_off); dfree(c, dst_off); dfree(c, out);
  };
  auto fail = [&](hipError_t e) {
    (void)rfxi::sync(c);  // (queued read-backs point at locals of this function: deliver them now)
    drop();
    if (e == hipSuccess) {
      rfxi::set_error("rfx_text_gather: out of device memory");
      return (int)RFX_E_NOMEM;
    }
    return hip_fail(e);
  };
  if (!tile_off || !line_start || !d_mask || !cnt || !sizes) return fail(hipSuccess);
  auto grid_of = [&](uint64_t items, int per_cu) { return dim3((unsigned)std::min<uint64_t>((items + 255) / 256, (uint64_t)c->n_cu * per_cu)); };
  // the mask upload (pageable host memory: the runtime has copied it out of `hitmask` when the call returns)
  hipError_t e = hipMemcpyAsync(d_mask, hitmask, (size_t)nw * 8, hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) e = rfxi::text_count_lines(c, arena, n, tile_off);
  if (e == hipSuccess) e = rfxi::text_line_starts(c, arena, n, tile_off, line_start, n_lines_want);
  if (e != hipSuccess) return fail(e);
  {
    // (an arena with fewer than 4 * n_records newlines leaves line starts unwritten: the sizes made of them are numbers
    // that nobody uses -- the newline count is checked before anything is sized by them)
    rfx_span sp(c, "k_gather_sizes");
    hipLaunchKernelGGL(k_gather_sizes, grid_of(nw, 16), dim3(256), 0, c->stream, line_start, d_mask, nw, tail, cnt, sizes);
  }
  rfxk::scan_tail(c, cnt, nw);
  rfxk::scan_tail(c, sizes, nw);
  uint64_t n_lines = 0, n_sel = 0, n_bytes = 0;
  unsigned char last = 0;
  e = queue_read(c, &n_lines, tile_off + n_tiles, 8);
  if (e == hipSuccess) e = queue_read(c, &n_sel, cnt + nw, 8);
  if (e == hipSuccess) e = queue_read(c, &n_bytes, sizes + nw, 8);
  if (e == hipSuccess) e = queue_read(c, &last, arena + n - 1, 1);
  if (e != hipSuccess) return fail(e);
  // the one wait: the newline count the arena is judged by, and the totals the result is sized by
  e = rfxi::sync(c);
  if (e != hipSuccess) return fail(e);
  if (n_lines != n_lines_want || last != '\n') {
    drop();
    return inval();
  }
  *bytes_out = n_bytes;
  if (n_selected) *n_selected = n_sel;
  if (n_bytes > cap) {
    drop();
    rfxi::set_error("rfx_text_gather: the output buffer is too small");
    return RFX_E_RANGE;
  }
  if (n_bytes == 0) {
    drop();
    return RFX_OK;
  }
  if (n_bytes > n) {  // (cannot be: the selected records are a subset of the arena)
    drop();
    rfxi::set_error("rfx_text_gather: the selection is larger than the text");
    return RFX_E_HIP;
  }
  src_off = (uint32_t*)dmalloc(c, (size_t)n_sel * 4);
  dst_off = (uint32_t*)dmalloc(c, ((size_t)n_sel + 1) * 4);
  out = (uint32_t*)dmalloc(c, ((size_t)n_bytes + 3) / 4 * 4);
  if (!src_off || !dst_off || !out) return fail(hipSuccess);
  {
    rfx_span sp(c, "k_gather_table");
    hipLaunchKernelGGL(k_gather_table, grid_of(nw, 16), dim3(256), 0, c->stream, line_start, d_mask, nw, tail, cnt, sizes, src_off,
                       dst_off);
  }
  {
    rfx_span sp(c, "k_gather_copy");
    hipLaunchKernelGGL(k_gather_copy, grid_of(n_bytes / 4 + 1, 32), dim3(256), 0, c->stream, (const uint32_t*)arena, src_off, dst_off,
                       (uint32_t)n_sel, (uint32_t)n_bytes, out);
  }
  e = hipGetLastError();
  // the bytes come back behind the kernels; the call returns when they are there
  if (e == hipSuccess) e = hipMemcpyAsync(host_out, out, (size_t)n_bytes, hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = rfxi::sync(c);
  if (e != hipSuccess) return fail(e);
  drop();
  return RFX_OK;
}
