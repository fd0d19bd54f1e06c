// BAM records found and packed on the device: what `samtools view -F 3328 X.bam | PassThroughSamCheck` (runRufus.sh:599,
// scripts/RunJellyForRUFUS.sh:28, src/PassThroughSamCheck.cpp:51-155) hands `jellyfish count`, from the inflated bytes
// rfx_text_append_bgzf leaves in a text arena.  The record layout is rfx_bam_core.h's, one source for host and device.
//
// A record is found only through its predecessor's block_size.  The arena is cut into tiles of T bytes (16 KiB;
// RFX_BAM_TILE: a power of two >= 256) and the chain is found by speculate, verify, repair:
//
//   k_bam_guess    a wave per tile t >= 1: 64 candidate offsets at a time from the tile's first byte, the first that
//                  bam_guess_ok accepts (a ballot) is in[t]; none: the sentinel, which equals no offset.  in[0] = skip.
//   k_bam_walk     a lane per tile: from in[t] along bam_next until the offset is >= the tile's end -> exit[t], and the
//                  number of records that START in the tile.  An entry behind the tile's end is passed through.
//   k_bam_repair   one round: every t >= 1 with in[t] != exit[t - 1] takes in[t] = exit[t - 1], is walked again and
//                  counted in `changed`.  exit[] is double-buffered, so a round reads only the round before.  The host
//                  repeats rounds until changed == 0 (4 bytes read back per round).
//
// Exact and finite: tile 0 is exact; after round r tiles 0 .. r are exact and never change again (in[r] is compared with
// an exit that is final); a fixed point has in[t] == exit[t - 1] everywhere, which IS the chain from `skip`.  A bad guess
// costs a round, never a result, and there are at most as many rounds as tiles.
//
//   scan of the counts, then
//   k_bam_starts   a lane per tile walks once more and writes rec_start[]; every record on the chain is checked with
//                  bam_valid, the lowest failing offset kept (atomicMin)
//
// rfx_bam_set_region (`samtools view X.bam CHR:BEG-END`, runRufus.sh -R):
//   k_bam_region   a thread per record: bam_in_region -> a byte per record that lives with rec_start[]; every kernel below
//                  that asks "kept?" asks bam_kept (rfx_bam_core.h): the flag test, and that byte while it is set
//
// rfx_bam_parse, shaped as rfx_select.hip:
//   k_bam_fields   a thread per record: flag, l_seq -> keep, code words, bases  -> three scans
//                  (+ the longest kept read and the histogram of lengths < 32: atomics on 33 counters)
//   k_bam_table    a thread per record: len[], word_off[], the sequence's byte offset and refID of the kept, at their rank
//                  (l_seq == 0: the read is the `*` samtools view prints, one base that is none of ACGT)
//   k_bam_runs     a thread per kept record: 1 where its refID differs from the kept record before it -> scan
//   k_bam_run_out  ... and the (first kept index, refID) pairs at their rank
//   k_bam_pack     a thread per OUTPUT code word: owner by binary search in word_off, its 16 source bytes by aligned
//                  dwords + alignbyte, bam_pack_word
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "rfx_bam_core.h"
#include "rfx_internal.h"

using rfxi::dfree;
using rfxi::dmalloc;
using rfxi::queue_read;

namespace {

constexpr uint32_t BAM_NONE = 0xFFFFFFFFu;  // no guess: an arena is shorter than 2^32 - 8192 bytes, so no offset equals it

int hip_fail(hipError_t e, const char* what) {
  char msg[256];
  snprintf(msg, sizeof msg, "%s: %s", what, hipGetErrorString(e));
  rfxi::set_error(msg);
  return RFX_E_HIP;
}

__global__ __launch_bounds__(256) void k_bam_guess(const uint8_t* __restrict__ b, uint64_t end, uint32_t tile, uint32_t n_tiles,
                                                    int32_t n_ref, uint32_t skip, int no_guess, uint32_t* __restrict__ in,
                                                    uint32_t* __restrict__ guess) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t t = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);  // (wave-uniform)
  if (t >= n_tiles) return;
  uint32_t g = BAM_NONE;
  if (t == 0) {
    g = skip;
  } else if (!no_guess) {
    const uint64_t lo = (uint64_t)t * tile, hi = min(lo + tile, end);
    for (uint64_t base = lo; base < hi; base += 64) {
      const uint64_t c = base + lane;
      const bool ok = c < hi && bam_guess_ok(b, c, end, n_ref);
      const unsigned long long vote = __ballot(ok);
      if (vote) {
        g = (uint32_t)(base + (uint32_t)(__ffsll((long long)vote) - 1));
        break;
      }
    }
  }
  if (lane == 0) {
    in[t] = g;
    guess[t] = g;
  }
}

__global__ __launch_bounds__(256) void k_bam_walk(const uint8_t* __restrict__ b, uint64_t end, uint32_t tile, uint32_t n_tiles,
                                                   const uint32_t* __restrict__ in, uint32_t* __restrict__ exit_out,
                                                   uint64_t* __restrict__ cnt) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_tiles) return;
  bam_no_visit nv;
  uint32_t n = 0;
  exit_out[t] = (uint32_t)bam_walk(b, in[t], min(((uint64_t)t + 1) * tile, end), end, &n, nv);
  cnt[t] = n;
}

__global__ __launch_bounds__(256) void k_bam_repair(const uint8_t* __restrict__ b, uint64_t end, uint32_t tile, uint32_t n_tiles,
                                                     uint32_t* __restrict__ in, const uint32_t* __restrict__ exit_prev,
                                                     uint32_t* __restrict__ exit_next, uint64_t* __restrict__ cnt,
                                                     uint32_t* __restrict__ changed) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_tiles) return;
  if (t == 0 || in[t] == exit_prev[t - 1]) {
    exit_next[t] = exit_prev[t];
    return;
  }
  const uint32_t entry = exit_prev[t - 1];
  in[t] = entry;
  bam_no_visit nv;
  uint32_t n = 0;
  exit_next[t] = (uint32_t)bam_walk(b, entry, min(((uint64_t)t + 1) * tile, end), end, &n, nv);
  cnt[t] = n;
  atomicAdd(changed, 1u);
}

struct bam_start_visit {
  const uint8_t* b;
  uint32_t* out;
  int32_t n_ref;
  uint32_t* first_bad;
  __device__ __forceinline__ void operator()(uint64_t p, uint32_t i) {
    out[i] = (uint32_t)p;
    if (bam_valid(b, p, n_ref) != BAM_OK) atomicMin(first_bad, (uint32_t)p);
  }
};

// info[0] = the lowest offset of a chain record that is not bam_valid (BAM_NONE: none), info[1] = guesses repair changed
__global__ __launch_bounds__(256) void k_bam_starts(const uint8_t* __restrict__ b, uint64_t end, uint32_t tile, uint32_t n_tiles,
                                                     int32_t n_ref, const uint32_t* __restrict__ in,
                                                     const uint32_t* __restrict__ guess, const uint64_t* __restrict__ off,
                                                     uint32_t* __restrict__ rec_start, uint32_t* __restrict__ info) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_tiles) return;
  bam_start_visit v{b, rec_start + off[t], n_ref, info};
  uint32_t n = 0;
  const uint64_t e = bam_walk(b, in[t], min(((uint64_t)t + 1) * tile, end), end, &n, v);  // (n == off[t + 1] - off[t])
  if (t == n_tiles - 1) rec_start[off[n_tiles]] = (uint32_t)e;                             // the cut
  if (guess[t] != in[t]) atomicAdd(&info[1], 1u);
}

// ---- rfx_bam_set_region -------------------------------------------------------------------------------------------------
// A thread per record: keep[r] = bam_in_region (a byte each; r < n_rec, the array's size).  *n_in: a ballot per wave, one
// 32-bit add of its population by lane 0 (an arena holds fewer than 2^30 records).  The loop's trip count is wave-uniform
// (it runs over the wave's first record), so every lane of a wave reaches the ballot.
__global__ __launch_bounds__(256) void k_bam_region(const uint8_t* __restrict__ b, const uint32_t* __restrict__ rec_start,
                                                     uint64_t n_rec, int32_t tid, int64_t beg, int64_t end,
                                                     uint8_t* __restrict__ keep, uint32_t* __restrict__ n_in) {
  const uint32_t lane = threadIdx.x & 63u;
  for (uint64_t r0 = (uint64_t)blockIdx.x * blockDim.x + (threadIdx.x & ~63u); r0 < n_rec; r0 += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t r = r0 + lane;
    bool in = false;
    if (r < n_rec) {
      in = bam_in_region(b, rec_start[r], tid, beg, end);
      keep[r] = in;
    }
    const unsigned long long vote = __ballot(in);
    if (lane == 0 && vote) atomicAdd(n_in, (uint32_t)__popcll(vote));
  }
}

// ---- rfx_bam_parse ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_bam_fields(const uint8_t* __restrict__ b, const uint32_t* __restrict__ rec_start,
                                                     uint64_t n_rec, uint32_t exclude, const uint8_t* __restrict__ region, uint64_t* __restrict__ cnt,
                                                     uint64_t* __restrict__ words, uint64_t* __restrict__ bases,
                                                     unsigned int* __restrict__ d_stat) {
  for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n_rec; r += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t p = rec_start[r];
    const bool keep = bam_kept(b, p, exclude, region, r);
    const uint32_t len = max((uint32_t)bam_l_seq(b, p), 1u);  // (>= 0: rfx_bam_settle has checked every record; 0: SEQ is `*`)
    cnt[r] = keep;
    words[r] = keep ? (len + 31u) / 32u : 0u;
    bases[r] = keep ? len : 0u;
    if (keep) {
      atomicMax(&d_stat[0], len);
      if (len < 32u) atomicAdd(&d_stat[1u + len], 1u);
    }
  }
}

__global__ __launch_bounds__(256) void k_bam_table(const uint8_t* __restrict__ b, const uint32_t* __restrict__ rec_start,
                                                    uint64_t n_rec, uint32_t exclude, const uint8_t* __restrict__ region, const uint64_t* __restrict__ cnt,
                                                    const uint64_t* __restrict__ words, uint32_t* __restrict__ out_len,
                                                    uint32_t* __restrict__ out_word_off, uint32_t* __restrict__ seq_at,
                                                    int32_t* __restrict__ ref_id) {
  for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n_rec; r += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t p = rec_start[r];
    if (!bam_kept(b, p, exclude, region, r)) continue;
    const uint32_t o = (uint32_t)cnt[r];  // (both totals are below 2^32: checked before this launch)
    const uint32_t l_seq = (uint32_t)bam_l_seq(b, p);
    out_len[o] = max(l_seq, 1u);  // (no sequence: samtools view prints `*`, one base that is none of ACGT)
    out_word_off[o] = (uint32_t)words[r];
    seq_at[o] = l_seq ? (uint32_t)bam_seq_offset(b, p) : BAM_NONE;
    ref_id[o] = bam_ref_id(b, p);
  }
}

__global__ __launch_bounds__(256) void k_bam_runs(const int32_t* __restrict__ ref_id, uint32_t n_kept, uint64_t* __restrict__ is_start) {
  for (uint64_t o = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; o < n_kept; o += (uint64_t)gridDim.x * blockDim.x)
    is_start[o] = o == 0 || ref_id[o] != ref_id[o - 1];
}

__global__ __launch_bounds__(256) void k_bam_run_out(const int32_t* __restrict__ ref_id, uint32_t n_kept,
                                                      const uint64_t* __restrict__ rank, uint32_t* __restrict__ runs) {
  for (uint64_t o = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; o < n_kept; o += (uint64_t)gridDim.x * blockDim.x)
    if (rank[o + 1] != rank[o]) {  // (the exclusive scan: a start is where the rank goes up)
      runs[2 * rank[o]] = (uint32_t)o;
      runs[2 * rank[o] + 1] = (uint32_t)ref_id[o];
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

// (five aligned dwords are read whatever the word needs: at most 19 bytes behind a sequence that lies inside the arena,
// which has 8 KiB behind its capacity)
__global__ __launch_bounds__(256) void k_bam_pack(const uint8_t* __restrict__ b, const uint32_t* __restrict__ word_off,
                                                   const uint32_t* __restrict__ len, const uint32_t* __restrict__ seq_at,
                                                   uint32_t n_kept, uint64_t n_words, uint64_t* __restrict__ codes,
                                                   uint32_t* __restrict__ acgt) {
  for (uint64_t x = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; x < n_words; x += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t o = owner_of(word_off, n_kept, (uint32_t)x);
    const uint32_t j = (uint32_t)x - word_off[o];
    const uint32_t nb = min(32u, len[o] - j * 32u);
    if (seq_at[o] == BAM_NONE) {  // `*`
      codes[x] = 0;
      acgt[x] = 0;
      continue;
    }
    const uint32_t src = seq_at[o] + j * 16u;
    const uint32_t* w = (const uint32_t*)(b + (src & ~3u));
    const uint32_t sh = src & 3u;
    const uint32_t d0 = w[0], d1 = w[1], d2 = w[2], d3 = w[3], d4 = w[4];
    const uint32_t v[4] = {__builtin_amdgcn_alignbyte(d1, d0, sh), __builtin_amdgcn_alignbyte(d2, d1, sh),
                           __builtin_amdgcn_alignbyte(d3, d2, sh), __builtin_amdgcn_alignbyte(d4, d3, sh)};
    uint64_t c;
    uint32_t m;
    bam_pack_word(v, nb, &c, &m);
    codes[x] = c;
    acgt[x] = m;
  }
}

uint32_t tile_bytes() {
  if (const char* e = getenv("RFX_BAM_TILE")) {
    const long long v = atoll(e);
    if (v >= 256 && v <= (1 << 30) && (v & (v - 1)) == 0) return (uint32_t)v;
  }
  return 16384;
}

}  // namespace

extern "C" {

int rfx_bam_settle(rfx_text* t, rfx_text* next, uint64_t skip, int32_t n_ref, uint64_t* n_records, uint64_t* carried) {
  static const char* const who = "rfx_bam_settle";
  if (!t || !carried || !n_records || next == t || n_ref < 0) return RFX_E_INVAL;
  *carried = 0;
  *n_records = 0;
  if (next && (rfx_text_bytes(next) != 0 || rfxi::text_ctx(next) != rfxi::text_ctx(t))) return RFX_E_INVAL;
  rfx_ctx* c = nullptr;
  const uint8_t* arena = nullptr;
  uint64_t n = 0;
  if (const int rc = rfxi::text_ready(t, &c, &arena, &n)) return rc;  // waits for the appends; a block that did not inflate
  if (skip > n) return RFX_E_INVAL;
  rfxi::text_bam& slot = rfxi::text_bam_of(t);
  if (slot.rec_start) dfree(c, slot.rec_start);
  if (slot.region) dfree(c, slot.region);
  slot = rfxi::text_bam();
  memset(c->bam_stats, 0, sizeof c->bam_stats);
  if (n == 0) {
    slot.settled = true;
    slot.n_ref = n_ref;
    return RFX_OK;
  }
  const uint32_t T = tile_bytes();
  const uint32_t n_tiles = (uint32_t)((n + T - 1) / T);
  const int no_guess = getenv("RFX_BAM_NO_GUESS") != nullptr && atoi(getenv("RFX_BAM_NO_GUESS")) != 0;
  uint32_t* u32s = (uint32_t*)dmalloc(c, ((size_t)4 * n_tiles + 4) * 4);  // in, guess, exit x 2, changed, info[2]
  uint64_t* cnt = (uint64_t*)dmalloc(c, ((size_t)n_tiles + 1) * 8);
  uint32_t* rec_start = nullptr;
  auto fail = [&](int rc, hipError_t e) {
    if (e != hipSuccess) hip_fail(e, who);
    (void)rfxi::sync(c);  // (queued read-backs point at locals of this function: deliver them now)
    dfree(c, u32s);
    dfree(c, cnt);
    dfree(c, rec_start);
    return rc;
  };
  if (!u32s || !cnt) return fail(RFX_E_NOMEM, hipSuccess);
  uint32_t *in = u32s, *guess = u32s + n_tiles, *ex[2] = {u32s + 2 * (size_t)n_tiles, u32s + 3 * (size_t)n_tiles};
  uint32_t *changed = u32s + 4 * (size_t)n_tiles, *info = changed + 1;
  const dim3 per_tile((n_tiles + 255) / 256), per_wave((n_tiles + 3) / 4);
  {
    rfx_span sp(c, "k_bam_guess");
    hipLaunchKernelGGL(k_bam_guess, per_wave, dim3(256), 0, c->stream, arena, n, T, n_tiles, n_ref, (uint32_t)skip, no_guess, in, guess);
  }
  {
    rfx_span sp(c, "k_bam_walk");
    hipLaunchKernelGGL(k_bam_walk, per_tile, dim3(256), 0, c->stream, arena, n, T, n_tiles, in, ex[0], cnt);
  }
  uint64_t rounds = 0;
  int cur = 0;
  for (;;) {
    hipError_t e = hipMemsetAsync(changed, 0, 4, c->stream);
    if (e != hipSuccess) return fail(RFX_E_HIP, e);
    {
      rfx_span sp(c, "k_bam_repair");
      hipLaunchKernelGGL(k_bam_repair, per_tile, dim3(256), 0, c->stream, arena, n, T, n_tiles, in, ex[cur], ex[cur ^ 1], cnt, changed);
    }
    uint32_t h_changed = 0;
    e = queue_read(c, &h_changed, changed, 4);
    if (e == hipSuccess) e = rfxi::sync(c);
    if (e != hipSuccess) return fail(RFX_E_HIP, e);
    cur ^= 1;
    if (!h_changed) break;
    if (++rounds > n_tiles) {  // (cannot happen: round r settles tile r)
      rfxi::set_error("rfx_bam_settle: the record chain did not settle");
      return fail(RFX_E_HIP, hipSuccess);
    }
  }
  rfxk::scan_tail(c, cnt, n_tiles);
  uint64_t n_rec = 0;
  uint32_t cut = 0;
  hipError_t e = queue_read(c, &n_rec, cnt + n_tiles, 8);
  if (e == hipSuccess) e = queue_read(c, &cut, ex[cur] + (n_tiles - 1), 4);
  if (e == hipSuccess) e = rfxi::sync(c);
  if (e != hipSuccess) return fail(RFX_E_HIP, e);
  if (cut > n || cut < skip || n_rec > n / 4) {
    rfxi::set_error("rfx_bam_settle: the cut lies outside the arena");
    return fail(RFX_E_HIP, hipSuccess);
  }
  rec_start = (uint32_t*)dmalloc(c, ((size_t)n_rec + 1) * 4);
  if (!rec_start) return fail(RFX_E_NOMEM, hipSuccess);
  const uint32_t info0[2] = {BAM_NONE, 0};
  e = hipMemcpyAsync(info, info0, 8, hipMemcpyHostToDevice, c->stream);
  if (e != hipSuccess) return fail(RFX_E_HIP, e);
  {
    rfx_span sp(c, "k_bam_starts");
    hipLaunchKernelGGL(k_bam_starts, per_tile, dim3(256), 0, c->stream, arena, n, T, n_tiles, n_ref, in, guess, cnt, rec_start, info);
  }
  uint32_t h_info[2] = {BAM_NONE, 0};
  e = queue_read(c, h_info, info, 8);
  if (e == hipSuccess) e = rfxi::sync(c);
  if (e != hipSuccess) return fail(RFX_E_HIP, e);
  c->bam_stats[0] = n_tiles;
  c->bam_stats[1] = h_info[1];
  c->bam_stats[2] = rounds;
  c->bam_stats[3] = n_rec;
  if (h_info[0] != BAM_NONE) {  // the lowest failing record: its fixed fields say why (a chain record is whole)
    uint8_t head[BAM_FIXED];
    memset(head, 0, sizeof head);
    const uint64_t have = std::min<uint64_t>(BAM_FIXED, n - h_info[0]);
    e = hipMemcpy(head, arena + h_info[0], have, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail(RFX_E_HIP, e);
    char msg[200];
    snprintf(msg, sizeof msg, "rfx_bam: record at byte %u: %s", h_info[0], bam_status_text(bam_valid(head, 0, n_ref)));
    rfxi::set_error(msg);
    return fail(RFX_E_FORMAT, hipSuccess);
  }
  // a first record that does not end inside an arena no further block fits into: no arena of this size ever holds it
  if (n_rec == 0 && cut < n && rfx_text_room(t) < 65536) {
    rfxi::set_error("rfx_bam_settle: the first record does not end inside a full arena");
    return fail(RFX_E_RANGE, hipSuccess);
  }
  if (const int rc = rfxi::text_cut(t, next, cut, carried, who)) return fail(rc, hipSuccess);
  dfree(c, u32s);
  dfree(c, cnt);
  slot.rec_start = rec_start;
  slot.n_records = n_rec;
  slot.n_ref = n_ref;
  slot.settled = true;
  *n_records = n_rec;
  return RFX_OK;
}

int rfx_bam_stats(const rfx_ctx* c, uint64_t out[4]) {
  if (!c || !out) return RFX_E_INVAL;
  memcpy(out, c->bam_stats, sizeof c->bam_stats);
  return RFX_OK;
}

int rfx_bam_set_region(rfx_text* t, int32_t tid, int64_t beg, int64_t end, uint64_t* n_in) {
  static const char* const who = "rfx_bam_set_region";
  if (n_in) *n_in = 0;
  if (!t || !n_in) return RFX_E_INVAL;
  rfxi::text_bam& slot = rfxi::text_bam_of(t);
  if (!slot.settled) {
    rfxi::set_error("rfx_bam_set_region: the arena has not been settled with rfx_bam_settle since its last reset");
    return RFX_E_INVAL;
  }
  rfx_ctx* c = nullptr;
  const uint8_t* arena = nullptr;
  uint64_t n = 0;
  if (const int rc = rfxi::text_ready(t, &c, &arena, &n)) return rc;
  const uint64_t R = slot.n_records;
  if (slot.region) dfree(c, slot.region);
  slot.region = nullptr;
  uint8_t* keep = (uint8_t*)dmalloc(c, std::max<uint64_t>(R, 1));
  uint32_t* d_in = (uint32_t*)dmalloc(c, 4);
  if (!keep || !d_in) {
    dfree(c, keep);
    dfree(c, d_in);
    rfxi::set_error("rfx_bam_set_region: out of device memory");
    return RFX_E_NOMEM;
  }
  if (R == 0) {
    dfree(c, d_in);
    slot.region = keep;
    return RFX_OK;
  }
  uint32_t h_in = 0;
  hipError_t e = hipMemsetAsync(d_in, 0, 4, c->stream);
  if (e == hipSuccess) {
    rfx_span sp(c, "k_bam_region");
    const dim3 grid((unsigned)std::min<uint64_t>((R + 255) / 256, (uint64_t)c->n_cu * 16));
    hipLaunchKernelGGL(k_bam_region, grid, dim3(256), 0, c->stream, arena, (const uint32_t*)slot.rec_start, R, tid, beg, end, keep, d_in);
    e = queue_read(c, &h_in, d_in, 4);
  }
  if (e == hipSuccess) e = rfxi::sync(c);
  else (void)rfxi::sync(c);  // (a queued read-back points at h_in: deliver it now)
  dfree(c, d_in);
  if (e != hipSuccess) {
    dfree(c, keep);
    return hip_fail(e, who);
  }
  slot.region = keep;
  *n_in = h_in;
  return RFX_OK;
}

rfx_reads* rfx_bam_parse(rfx_text* t, uint32_t exclude_flags, uint32_t* ref_runs, uint64_t cap, uint64_t* n_runs) {
  static const char* const who = "rfx_bam_parse";
  char msg[256];
  if (n_runs) *n_runs = 0;
  if (!t || !n_runs || (!ref_runs && cap)) {
    rfxi::set_error("rfx_bam_parse: RFX_E_INVAL: a NULL argument");
    return nullptr;
  }
  rfxi::text_bam& slot = rfxi::text_bam_of(t);
  if (!slot.settled) {
    rfxi::set_error("rfx_bam_parse: RFX_E_INVAL: the arena has not been settled with rfx_bam_settle since its last reset");
    return nullptr;
  }
  rfx_ctx* c = nullptr;
  const uint8_t* arena = nullptr;
  uint64_t n = 0;
  if (rfxi::text_ready(t, &c, &arena, &n) != RFX_OK) return nullptr;
  const uint64_t R = slot.n_records;
  rfx_reads* r = new rfx_reads();
  memset(r, 0, sizeof *r);
  r->gen = rfx_next_reads_gen();
  r->ctx = c;
  uint64_t* cnt = (uint64_t*)dmalloc(c, (R + 1) * 8);
  uint64_t* words = (uint64_t*)dmalloc(c, (R + 1) * 8);
  uint64_t* bases = (uint64_t*)dmalloc(c, (R + 1) * 8);
  unsigned int* d_stat = (unsigned int*)dmalloc(c, 33 * 4);  // [0] longest kept read, [1 + l] kept reads of l < 32 bases
  uint32_t* seq_at = nullptr;
  int32_t* ref_id = nullptr;
  uint64_t* run_rank = nullptr;
  uint32_t* d_runs = nullptr;
  auto fail = [&](hipError_t e, const char* code, const char* text) -> rfx_reads* {
    snprintf(msg, sizeof msg, "%s: %s: %s", who, code, e != hipSuccess ? hipGetErrorString(e) : text);
    (void)rfxi::sync(c);  // (queued read-backs point at locals of this function: deliver them now)
    rfxi::set_error(msg);
    dfree(c, cnt); dfree(c, words); dfree(c, bases); dfree(c, d_stat); dfree(c, seq_at); dfree(c, ref_id); dfree(c, run_rank);
    dfree(c, d_runs);
    rfx_reads_free(r);
    return nullptr;
  };
  if (!cnt || !words || !bases || !d_stat) return fail(hipSuccess, "RFX_E_NOMEM", "out of device memory");
  auto grid_of = [&](uint64_t m, int per_cu) { return dim3((unsigned)std::min<uint64_t>((m + 255) / 256, (uint64_t)c->n_cu * per_cu)); };
  uint64_t totals[3] = {0, 0, 0};  // kept reads, words, bases
  unsigned int h_stat[33];
  memset(h_stat, 0, sizeof h_stat);
  if (R) {
    hipError_t e = hipMemsetAsync(d_stat, 0, 33 * 4, c->stream);
    if (e != hipSuccess) return fail(e, "RFX_E_HIP", "");
    {
      rfx_span sp(c, "k_bam_fields");
      hipLaunchKernelGGL(k_bam_fields, grid_of(R, 16), dim3(256), 0, c->stream, arena, slot.rec_start, R, exclude_flags, (const uint8_t*)slot.region, cnt, words,
                         bases, d_stat);
    }
    rfxk::scan_tail(c, cnt, R);
    rfxk::scan_tail(c, words, R);
    rfxk::scan_tail(c, bases, R);
    e = queue_read(c, &totals[0], cnt + R, 8);
    if (e == hipSuccess) e = queue_read(c, &totals[1], words + R, 8);
    if (e == hipSuccess) e = queue_read(c, &totals[2], bases + R, 8);
    if (e == hipSuccess) e = queue_read(c, h_stat, d_stat, sizeof h_stat);
    if (e == hipSuccess) e = rfxi::sync(c);  // the first wait: the totals the result is allocated by
    if (e != hipSuccess) return fail(e, "RFX_E_HIP", "");
  }
  const uint64_t S = totals[0], W = totals[1];
  if (S >= (1ull << 32) || W >= (1ull << 32)) return fail(hipSuccess, "RFX_E_RANGE", "the block would reach 2^32 reads or words");
  r->n = (uint32_t)S;
  r->n_words = W;
  r->n_bases = totals[2];
  r->max_len = h_stat[0];
  for (int l = 0; l < 32; ++l) r->short_cnt[l] = h_stat[1 + l];
  r->codes = (uint64_t*)dmalloc(c, std::max<uint64_t>(W, 1) * 8);
  r->acgt = (uint32_t*)dmalloc(c, std::max<uint64_t>(W, 1) * 4);
  r->word_off = (uint32_t*)dmalloc(c, ((size_t)S + 1) * 4);
  r->len = (uint32_t*)dmalloc(c, std::max<uint64_t>(S, 1) * 4);
  seq_at = (uint32_t*)dmalloc(c, std::max<uint64_t>(S, 1) * 4);
  ref_id = (int32_t*)dmalloc(c, std::max<uint64_t>(S, 1) * 4);
  run_rank = (uint64_t*)dmalloc(c, (S + 1) * 8);
  if (!r->codes || !r->acgt || !r->word_off || !r->len || !seq_at || !ref_id || !run_rank)
    return fail(hipSuccess, "RFX_E_NOMEM", "out of device memory");
  const uint32_t w_end = (uint32_t)W;
  uint64_t runs = 0;
  hipError_t e = hipMemcpyAsync(r->word_off + S, &w_end, 4, hipMemcpyHostToDevice, c->stream);  // (w_end lives until the wait below)
  if (e != hipSuccess) return fail(e, "RFX_E_HIP", "");
  if (S) {
    {
      rfx_span sp(c, "k_bam_table");
      hipLaunchKernelGGL(k_bam_table, grid_of(R, 16), dim3(256), 0, c->stream, arena, slot.rec_start, R, exclude_flags, (const uint8_t*)slot.region, cnt, words,
                         r->len, r->word_off, seq_at, ref_id);
    }
    {
      rfx_span sp(c, "k_bam_runs");
      hipLaunchKernelGGL(k_bam_runs, grid_of(S, 16), dim3(256), 0, c->stream, ref_id, (uint32_t)S, run_rank);
    }
    rfxk::scan_tail(c, run_rank, S);
    e = queue_read(c, &runs, run_rank + S, 8);
    if (e != hipSuccess) return fail(e, "RFX_E_HIP", "");
    if (W) {
      rfx_span sp(c, "k_bam_pack");
      hipLaunchKernelGGL(k_bam_pack, grid_of(W, 32), dim3(256), 0, c->stream, arena, r->word_off, r->len, seq_at, (uint32_t)S, W,
                         r->codes, r->acgt);
    }
  }
  e = rfxi::sync(c);  // the second wait: the block is packed, the number of runs is known
  if (e != hipSuccess) return fail(e, "RFX_E_HIP", "");
  *n_runs = runs;
  if (runs > cap) return fail(hipSuccess, "RFX_E_RANGE", "more reference runs than the caller has room for");
  if (runs) {
    d_runs = (uint32_t*)dmalloc(c, runs * 8);
    if (!d_runs) return fail(hipSuccess, "RFX_E_NOMEM", "out of device memory");
    {
      rfx_span sp(c, "k_bam_run_out");
      hipLaunchKernelGGL(k_bam_run_out, grid_of(S, 16), dim3(256), 0, c->stream, ref_id, (uint32_t)S, run_rank, d_runs);
    }
    e = hipMemcpyAsync(ref_runs, d_runs, runs * 8, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = rfxi::sync(c);
    if (e != hipSuccess) return fail(e, "RFX_E_HIP", "");
  }
  dfree(c, cnt); dfree(c, words); dfree(c, bases); dfree(c, d_stat); dfree(c, seq_at); dfree(c, ref_id); dfree(c, run_rank);
  dfree(c, d_runs);
  return r;
}

}  // extern "C"

// ---- the subject's hit pairs straight from the BAM (RUFUS.Filter --bam) ------------------------------------------------
// Replaces `samtools view -F 3328 X.bam | PassThroughSamCheck.stranded | RUFUS.Filter` (runRufus.sh:964-967).
//
// rfx_bam_parse_filter, rfx_bam_parse's shape with the STRANDED FILTER form of rfx_bam_core.h:
//   k_bamf_fields  a thread per record: keep, bam_filter_len (a reverse record: its surviving nibbles) -> three scans
//   k_bamf_table   a thread per record: len[], word_off[], the record's offset and refID of the kept, at their rank
//   k_bam_runs / k_bam_run_out   as above
//   k_bamf_pack    a thread per OUTPUT code word: owner by binary search in word_off, bam_filter_word
//
// The pull (pass 2 of the tool: no pack, no scan), over the KEPT records of a settled arena -- kept_of: k_bam_keep, a scan,
// k_bam_kept_at = the offset of kept record o:
//   k_bam_hashes   a thread per kept record: bam_name_hash of the records a mask selects, at their rank among the selected
//                  (the rank of a mask word's first bit comes with the mask: the mask is the host's)
//   k_bam_mark     a wave per 64 kept records = one mask word: bam_name_hash, a probe of the open-addressed table, a ballot
//   k_bamg_sizes / k_bamg_table   rfx_gather.hip's two, with a record's bytes = 4 + block_size -> k_gather_copy
namespace {

__global__ __launch_bounds__(256) void k_bamf_fields(const uint8_t* __restrict__ b, const uint32_t* __restrict__ rec_start,
                                                      uint64_t n_rec, uint32_t exclude, const uint8_t* __restrict__ region, uint64_t* __restrict__ cnt,
                                                      uint64_t* __restrict__ words, uint64_t* __restrict__ bases,
                                                      unsigned int* __restrict__ d_stat) {
  for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n_rec; r += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t p = rec_start[r];
    const bool keep = bam_kept(b, p, exclude, region, r);
    const uint32_t len = keep ? bam_filter_len(b, p) : 0u;
    cnt[r] = keep;
    words[r] = (len + 31u) / 32u;
    bases[r] = len;
    if (keep) {
      atomicMax(&d_stat[0], len);
      if (len < 32u) atomicAdd(&d_stat[1u + len], 1u);
    }
  }
}

// (cnt, words: scanned; bases: scanned too, so a record's length is the difference of two entries)
__global__ __launch_bounds__(256) void k_bamf_table(const uint8_t* __restrict__ b, const uint32_t* __restrict__ rec_start,
                                                     uint64_t n_rec, uint32_t exclude, const uint8_t* __restrict__ region, const uint64_t* __restrict__ cnt,
                                                     const uint64_t* __restrict__ words, const uint64_t* __restrict__ bases,
                                                     uint32_t* __restrict__ out_len, uint32_t* __restrict__ out_word_off,
                                                     uint32_t* __restrict__ rec_at, int32_t* __restrict__ ref_id) {
  for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n_rec; r += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t p = rec_start[r];
    if (!bam_kept(b, p, exclude, region, r)) continue;
    const uint32_t o = (uint32_t)cnt[r];  // (both totals are below 2^32: checked before this launch)
    out_len[o] = (uint32_t)(bases[r + 1] - bases[r]);
    out_word_off[o] = (uint32_t)words[r];
    rec_at[o] = (uint32_t)p;
    ref_id[o] = bam_ref_id(b, p);
  }
}

__global__ __launch_bounds__(256) void k_bamf_pack(const uint8_t* __restrict__ b, const uint32_t* __restrict__ word_off,
                                                    const uint32_t* __restrict__ len, const uint32_t* __restrict__ rec_at,
                                                    uint32_t n_kept, uint64_t n_words, int min_q, uint64_t* __restrict__ codes,
                                                    uint32_t* __restrict__ good) {
  for (uint64_t x = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; x < n_words; x += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t o = owner_of(word_off, n_kept, (uint32_t)x);  // (a read of 0 bases owns no word: the LAST o with off <= x)
    uint64_t c;
    uint32_t g;
    bam_filter_word(b, rec_at[o], (uint32_t)x - word_off[o], len[o], min_q, &c, &g);
    codes[x] = c;
    good[x] = g;
  }
}

__global__ __launch_bounds__(256) void k_bam_keep(const uint8_t* __restrict__ b, const uint32_t* __restrict__ rec_start,
                                                   uint64_t n_rec, uint32_t exclude, const uint8_t* __restrict__ region, uint64_t* __restrict__ cnt) {
  for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n_rec; r += (uint64_t)gridDim.x * blockDim.x)
    cnt[r] = bam_kept(b, rec_start[r], exclude, region, r);
}

__global__ __launch_bounds__(256) void k_bam_kept_at(const uint32_t* __restrict__ rec_start, uint64_t n_rec,
                                                      const uint64_t* __restrict__ cnt, uint32_t* __restrict__ kept_at) {
  for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n_rec; r += (uint64_t)gridDim.x * blockDim.x)
    if (cnt[r + 1] != cnt[r]) kept_at[cnt[r]] = rec_start[r];
}

// mask == nullptr: every kept record, at its own index
__global__ __launch_bounds__(256) void k_bam_hashes(const uint8_t* __restrict__ b, const uint32_t* __restrict__ kept_at,
                                                     uint64_t n_kept, const uint64_t* __restrict__ mask,
                                                     const uint64_t* __restrict__ word_rank, uint64_t* __restrict__ out) {
  for (uint64_t o = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; o < n_kept; o += (uint64_t)gridDim.x * blockDim.x) {
    uint64_t at = o;
    if (mask) {
      const uint64_t m = mask[o >> 6], bit = 1ull << (o & 63u);
      if (!(m & bit)) continue;
      at = word_rank[o >> 6] + (uint64_t)__popcll(m & (bit - 1ull));
    }
    out[at] = bam_name_hash(b, kept_at[o]);
  }
}

// The table: `slots` (a power of two) keys, 0 = empty, linear probing from nameset_slot; a key 0 is kept beside it.
__host__ __device__ __forceinline__ uint64_t nameset_slot(uint64_t key, uint64_t slots) {
  return ((key ^ (key >> 32)) * 0x9E3779B97F4A7C15ull >> 20) & (slots - 1ull);
}

// blockDim = 256 = four waves; wave w of the grid takes mask words w, w + waves, ...: 64 kept records each, a lane a record
__global__ __launch_bounds__(256) void k_bam_mark(const uint8_t* __restrict__ b, const uint32_t* __restrict__ kept_at, uint64_t n_kept,
                                                   const uint64_t* __restrict__ table, uint64_t slots, int has_zero,
                                                   uint64_t* __restrict__ mask_out, unsigned long long* __restrict__ n_marked) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t waves = (uint64_t)gridDim.x * (blockDim.x >> 6), nw = (n_kept + 63) / 64;
  for (uint64_t w = (uint64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); w < nw; w += waves) {  // (wave-uniform)
    const uint64_t o = w * 64 + lane;
    bool in = false;
    if (o < n_kept) {
      const uint64_t h = bam_name_hash(b, kept_at[o]);
      if (h == 0) {
        in = has_zero != 0;
      } else {
        for (uint64_t s = nameset_slot(h, slots);; s = (s + 1) & (slots - 1ull)) {  // (ends: the table is at most half full)
          const uint64_t key = table[s];
          if (key == h) in = true;
          if (key == h || key == 0) break;
        }
      }
    }
    const unsigned long long vote = __ballot(in);
    if (lane == 0) {
      mask_out[w] = vote;
      if (vote) atomicAdd(n_marked, (unsigned long long)__popcll(vote));
    }
  }
}

__device__ __forceinline__ uint32_t record_bytes(const uint8_t* b, uint32_t p) { return 4u + bam_block_size(b, p); }

__global__ __launch_bounds__(256) void k_bamg_sizes(const uint8_t* __restrict__ b, const uint32_t* __restrict__ kept_at,
                                                     const uint64_t* __restrict__ mask, uint32_t nw, uint64_t tail,
                                                     uint64_t* __restrict__ cnt, uint64_t* __restrict__ bytes) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nw; i += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t w = (uint32_t)i;
    uint64_t m = mask[w];
    if (w == nw - 1u) m &= tail;  // bits at and above the kept count are ignored
    uint64_t nbytes = 0;
    for (uint32_t h = 0; h < 2u; ++h) {
      uint32_t bits = h ? (uint32_t)(m >> 32) : (uint32_t)m;
      while (bits) {
        const uint32_t bit = (uint32_t)__ffs(bits) - 1u;
        bits &= bits - 1u;
        nbytes += record_bytes(b, kept_at[w * 64u + h * 32u + bit]);
      }
    }
    cnt[w] = (uint32_t)__popcll(m);
    bytes[w] = nbytes;
  }
}

// cnt / bytes: the scanned arrays (positions in the result)
__global__ __launch_bounds__(256) void k_bamg_table(const uint8_t* __restrict__ b, const uint32_t* __restrict__ kept_at,
                                                     const uint64_t* __restrict__ mask, uint32_t nw, uint64_t tail,
                                                     const uint64_t* __restrict__ cnt, const uint64_t* __restrict__ bytes,
                                                     uint32_t* __restrict__ src_off, uint32_t* __restrict__ dst_off) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nw; i += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t w = (uint32_t)i;
    uint64_t m = mask[w];
    if (w == nw - 1u) m &= tail;
    uint32_t o = (uint32_t)cnt[w], at = (uint32_t)bytes[w];  // (both totals are below 2^32: the arena is)
    for (uint32_t h = 0; h < 2u; ++h) {
      uint32_t bits = h ? (uint32_t)(m >> 32) : (uint32_t)m;
      while (bits) {
        const uint32_t bit = (uint32_t)__ffs(bits) - 1u;
        bits &= bits - 1u;
        const uint32_t s = kept_at[w * 64u + h * 32u + bit];
        src_off[o] = s;
        dst_off[o] = at;
        ++o;
        at += record_bytes(b, s);
      }
    }
    if (w == nw - 1u) dst_off[o] = at;  // dst_off[n_sel] = all bytes
  }
}

// ---- the hit records of an arena with their hit counts (RUFUS.Filter.single --bam) ----------------------------------------
// Replaces `samtools view -F 3328 X.bam | PassThroughSamCheck.stranded.se CHR | RUFUS.Filter.single ...` (runRufus.sh:1031-1032).
// What becomes of a record depends on that record alone (src/PassThroughSamCheck.stranded.se.cpp:155-203 prints it,
// src/RUFUS.Filter.ss.cpp:164-203 scans it -- `i < length()`: the last base IS examined -- and writes it when its count
// reaches the threshold, :194), so one pass does it: rfx_bam_parse_filter's block goes through the filter in its counting
// mode, and the selection is made from the COUNTS (the filter's own mask has undefined bits at and above n, and the pair
// filter's mask-only mode leaves no counts at all):
//   k_bamh_pick    k_bam_mark's shape -- a wave per 64 kept records, a lane a record: the ballot of `count >= thresh`, the
//                  selected records' 4 + block_size summed over the wave by shuffles -> cnt[w], bytes[w]   -> two scans
//   k_bamh_table   the same ballot again; a selected lane's rank = the votes below it (mbcnt), its offset = an in-wave
//                  exclusive prefix of the selected sizes (six shuffle steps, every lane taking part): source offset,
//                  destination offset, count and kept index at cnt[w] + rank                               -> k_gather_copy
// No LDS, no atomics; the trip count of both loops is wave-uniform, so every lane reaches every ballot and shuffle; lanes
// at and above n_kept vote 0 and bring 0 bytes.  hits[o] and kept_at[o] are read for o < n_kept only, a record's size only
// through bam_block_size inside a record the settle has checked.  All totals are below 2^32: an arena is.
__global__ __launch_bounds__(256) void k_bamh_pick(const uint8_t* __restrict__ b, const uint32_t* __restrict__ kept_at,
                                                    const uint32_t* __restrict__ hits, uint64_t n_kept, int thresh,
                                                    uint64_t* __restrict__ cnt, uint64_t* __restrict__ bytes) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t waves = (uint64_t)gridDim.x * (blockDim.x >> 6), nw = (n_kept + 63) / 64;
  for (uint64_t w = (uint64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); w < nw; w += waves) {  // (wave-uniform)
    const uint64_t o = w * 64 + lane;
    const bool sel = o < n_kept && (int)hits[o] >= thresh;
    const unsigned long long vote = __ballot(sel);
    uint32_t nb = sel ? record_bytes(b, kept_at[o]) : 0u;
    for (int d = 32; d; d >>= 1) nb += __shfl_xor(nb, d);
    if (lane == 0) {
      cnt[w] = (uint32_t)__popcll(vote);
      bytes[w] = nb;
    }
  }
}

// cnt / bytes: the scanned arrays (positions in the result)
__global__ __launch_bounds__(256) void k_bamh_table(const uint8_t* __restrict__ b, const uint32_t* __restrict__ kept_at,
                                                     const uint32_t* __restrict__ hits, uint64_t n_kept, int thresh,
                                                     const uint64_t* __restrict__ cnt, const uint64_t* __restrict__ bytes,
                                                     uint32_t* __restrict__ src_off, uint32_t* __restrict__ dst_off,
                                                     uint32_t* __restrict__ hits_sel, uint32_t* __restrict__ index_sel) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t waves = (uint64_t)gridDim.x * (blockDim.x >> 6), nw = (n_kept + 63) / 64;
  for (uint64_t w = (uint64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); w < nw; w += waves) {  // (wave-uniform)
    const uint64_t o = w * 64 + lane;
    uint32_t h = 0, s = 0;
    bool sel = false;
    if (o < n_kept) {
      h = hits[o];
      sel = (int)h >= thresh;
      if (sel) s = kept_at[o];
    }
    const unsigned long long vote = __ballot(sel);
    const uint32_t nb = sel ? record_bytes(b, s) : 0u;
    uint32_t upto = nb;  // the inclusive prefix of the sizes: lane l adds what lies d lanes below it, d = 1, 2, .. 32
    for (uint32_t d = 1; d < 64u; d <<= 1) {
      const uint32_t below = __shfl_up(upto, d);
      if (lane >= d) upto += below;
    }
    const uint32_t first = (uint32_t)cnt[w], at0 = (uint32_t)bytes[w];  // (both totals are below 2^32: the arena is)
    if (sel) {
      const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(vote >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)vote, 0u));
      src_off[first + rank] = s;
      dst_off[first + rank] = at0 + upto - nb;
      hits_sel[first + rank] = h;
      index_sel[first + rank] = (uint32_t)o;
    }
    if (w == nw - 1 && lane == 63u) dst_off[first + (uint32_t)__popcll(vote)] = at0 + upto;  // dst_off[n_sel] = all bytes
  }
}

// a kept record's address: where its block_size field lies in the arena, and the bytes from there to its end
__global__ __launch_bounds__(256) void k_bam_locate(const uint8_t* __restrict__ b, const uint32_t* __restrict__ kept_at, uint64_t n_kept,
                                                     uint32_t* __restrict__ start_out, uint32_t* __restrict__ bytes_out) {
  for (uint64_t o = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; o < n_kept; o += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t p = kept_at[o];
    start_out[o] = p;
    bytes_out[o] = record_bytes(b, p);
  }
}

// Entry i of a fetch list names a record when it holds the fixed fields, lies inside the arena's `used` bytes and begins
// with its own length (read bytewise: any residue).  *first_bad = the lowest i that does not; sizes[i] = bytes[i] for the scan.
__global__ __launch_bounds__(256) void k_fetch_check(const uint8_t* __restrict__ b, uint64_t used, const uint32_t* __restrict__ start,
                                                      const uint32_t* __restrict__ bytes, uint64_t n, uint32_t* __restrict__ first_bad,
                                                      uint64_t* __restrict__ sizes) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t s = start[i], nb = bytes[i];
    sizes[i] = nb;
    bool ok = nb >= BAM_FIXED && (uint64_t)s + nb <= used;
    if (ok) ok = bam_block_size(b, s) == nb - 4u;  // (s + 4 <= s + nb <= used)
    if (!ok) atomicMin(first_bad, (uint32_t)i);
  }
}

// off: the scanned sizes from the run's first entry on (n + 1 of them); destinations count from the run's first byte
__global__ __launch_bounds__(256) void k_fetch_table(const uint32_t* __restrict__ start, const uint64_t* __restrict__ off, uint32_t n,
                                                      uint32_t* __restrict__ src_off, uint32_t* __restrict__ dst_off) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
    src_off[i] = start[i];
    dst_off[i] = (uint32_t)(off[i] - off[0]);  // (a run is at most 1 GiB, or one record of an arena below 4 GiB)
    if (i == n - 1u) dst_off[n] = (uint32_t)(off[n] - off[0]);
  }
}

// k_bam_mark's shape over an array of hashes: wave w of the grid takes mask words w, w + waves, ...; a piece holds fewer
// than 2^32 hashes, so its set bits are counted with a 32-bit atomic
__global__ __launch_bounds__(256) void k_nameset_mark(const uint64_t* __restrict__ hashes, uint64_t n, const uint64_t* __restrict__ table,
                                                       uint64_t slots, int has_zero, uint64_t* __restrict__ mask_out,
                                                       uint32_t* __restrict__ n_marked) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t waves = (uint64_t)gridDim.x * (blockDim.x >> 6), nw = (n + 63) / 64;
  for (uint64_t w = (uint64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); w < nw; w += waves) {  // (wave-uniform)
    const uint64_t o = w * 64 + lane;
    bool in = false;
    if (o < n) {
      const uint64_t h = hashes[o];
      if (h == 0) {
        in = has_zero != 0;
      } else {
        for (uint64_t s = nameset_slot(h, slots);; s = (s + 1) & (slots - 1ull)) {  // (ends: the table is at most half full)
          const uint64_t key = table[s];
          if (key == h) in = true;
          if (key == h || key == 0) break;
        }
      }
    }
    const unsigned long long vote = __ballot(in);
    if (lane == 0) {
      mask_out[w] = vote;
      if (vote) atomicAdd(n_marked, (uint32_t)__popcll(vote));
    }
  }
}

// What the three pull calls begin with: the arena settled and ready, kept_at[o] = the offset of kept record o (device,
// dmalloc: the caller frees it; nullptr for 0 kept records), *n_kept.  One wait.
struct kept_view {
  rfx_ctx* c = nullptr;
  const uint8_t* arena = nullptr;
  uint64_t n = 0, n_kept = 0;
  uint32_t* kept_at = nullptr;
};
int kept_of(rfx_text* t, uint32_t exclude, const char* who, kept_view* v) {
  char msg[200];
  rfxi::text_bam& slot = rfxi::text_bam_of(t);
  if (!slot.settled) {
    snprintf(msg, sizeof msg, "%s: the arena has not been settled with rfx_bam_settle since its last reset", who);
    rfxi::set_error(msg);
    return RFX_E_INVAL;
  }
  if (const int rc = rfxi::text_ready(t, &v->c, &v->arena, &v->n)) return rc;
  const uint64_t R = slot.n_records;
  if (R == 0) return RFX_OK;
  rfx_ctx* c = v->c;
  uint64_t* cnt = (uint64_t*)dmalloc(c, (R + 1) * 8);
  auto fail = [&](int rc, hipError_t e) {
    snprintf(msg, sizeof msg, "%s: %s", who, e != hipSuccess ? hipGetErrorString(e) : "out of device memory");
    (void)rfxi::sync(c);
    rfxi::set_error(msg);
    dfree(c, cnt);
    dfree(c, v->kept_at);
    v->kept_at = nullptr;
    return rc;
  };
  if (!cnt) return fail(RFX_E_NOMEM, hipSuccess);
  const dim3 grid((unsigned)std::min<uint64_t>((R + 255) / 256, (uint64_t)c->n_cu * 16));
  {
    rfx_span sp(c, "k_bam_keep");
    hipLaunchKernelGGL(k_bam_keep, grid, dim3(256), 0, c->stream, v->arena, slot.rec_start, R, exclude, (const uint8_t*)slot.region, cnt);
  }
  rfxk::scan_tail(c, cnt, R);
  hipError_t e = queue_read(c, &v->n_kept, cnt + R, 8);
  if (e == hipSuccess) e = rfxi::sync(c);
  if (e != hipSuccess) return fail(RFX_E_HIP, e);
  if (v->n_kept) {
    v->kept_at = (uint32_t*)dmalloc(c, (size_t)v->n_kept * 4);
    if (!v->kept_at) return fail(RFX_E_NOMEM, hipSuccess);
    rfx_span sp(c, "k_bam_kept_at");
    hipLaunchKernelGGL(k_bam_kept_at, grid, dim3(256), 0, c->stream, slot.rec_start, R, cnt, v->kept_at);
  }
  e = rfxi::sync(c);  // (cnt is read by the launch: it is freed behind it)
  if (e != hipSuccess) return fail(RFX_E_HIP, e);
  dfree(c, cnt);
  return RFX_OK;
}

int pull_fail(rfx_ctx* c, const char* who, int rc, hipError_t e, const char* text) {
  char msg[256];
  snprintf(msg, sizeof msg, "%s: %s", who, e != hipSuccess ? hipGetErrorString(e) : text);
  if (c) (void)rfxi::sync(c);
  rfxi::set_error(msg);
  return rc;
}

}  // namespace

struct rfx_nameset {
  rfx_ctx* ctx;
  uint64_t* table;  // device: `slots` keys, 0 = empty
  uint64_t slots, n;
  int has_zero;
};

extern "C" {

rfx_reads* rfx_bam_parse_filter(rfx_text* t, uint32_t exclude_flags, int min_q, uint32_t* ref_runs, uint64_t cap, uint64_t* n_runs) {
  static const char* const who = "rfx_bam_parse_filter";
  char msg[256];
  if (n_runs) *n_runs = 0;
  if (!t || !n_runs || (!ref_runs && cap)) {
    rfxi::set_error("rfx_bam_parse_filter: RFX_E_INVAL: a NULL argument");
    return nullptr;
  }
  rfxi::text_bam& slot = rfxi::text_bam_of(t);
  if (!slot.settled) {
    rfxi::set_error("rfx_bam_parse_filter: RFX_E_INVAL: the arena has not been settled with rfx_bam_settle since its last reset");
    return nullptr;
  }
  rfx_ctx* c = nullptr;
  const uint8_t* arena = nullptr;
  uint64_t n = 0;
  if (rfxi::text_ready(t, &c, &arena, &n) != RFX_OK) return nullptr;
  const uint64_t R = slot.n_records;
  rfx_reads* r = new rfx_reads();
  memset(r, 0, sizeof *r);
  r->gen = rfx_next_reads_gen();
  r->ctx = c;
  uint64_t* cnt = (uint64_t*)dmalloc(c, (R + 1) * 8);
  uint64_t* words = (uint64_t*)dmalloc(c, (R + 1) * 8);
  uint64_t* bases = (uint64_t*)dmalloc(c, (R + 1) * 8);
  unsigned int* d_stat = (unsigned int*)dmalloc(c, 33 * 4);  // [0] longest kept read, [1 + l] kept reads of l < 32 bases
  uint32_t* rec_at = nullptr;
  int32_t* ref_id = nullptr;
  uint64_t* run_rank = nullptr;
  uint32_t* d_runs = nullptr;
  auto fail = [&](hipError_t e, const char* code, const char* text) -> rfx_reads* {
    snprintf(msg, sizeof msg, "%s: %s: %s", who, code, e != hipSuccess ? hipGetErrorString(e) : text);
    (void)rfxi::sync(c);  // (queued read-backs point at locals of this function: deliver them now)
    rfxi::set_error(msg);
    dfree(c, cnt); dfree(c, words); dfree(c, bases); dfree(c, d_stat); dfree(c, rec_at); dfree(c, ref_id); dfree(c, run_rank);
    dfree(c, d_runs);
    rfx_reads_free(r);
    return nullptr;
  };
  if (!cnt || !words || !bases || !d_stat) return fail(hipSuccess, "RFX_E_NOMEM", "out of device memory");
  auto grid_of = [&](uint64_t m, int per_cu) { return dim3((unsigned)std::min<uint64_t>((m + 255) / 256, (uint64_t)c->n_cu * per_cu)); };
  uint64_t totals[3] = {0, 0, 0};  // kept reads, words, bases
  unsigned int h_stat[33];
  memset(h_stat, 0, sizeof h_stat);
  if (R) {
    hipError_t e = hipMemsetAsync(d_stat, 0, 33 * 4, c->stream);
    if (e != hipSuccess) return fail(e, "RFX_E_HIP", "");
    {
      rfx_span sp(c, "k_bamf_fields");
      hipLaunchKernelGGL(k_bamf_fields, grid_of(R, 16), dim3(256), 0, c->stream, arena, slot.rec_start, R, exclude_flags, (const uint8_t*)slot.region, cnt, words,
                         bases, d_stat);
    }
    rfxk::scan_tail(c, cnt, R);
    rfxk::scan_tail(c, words, R);
    rfxk::scan_tail(c, bases, R);
    e = queue_read(c, &totals[0], cnt + R, 8);
    if (e == hipSuccess) e = queue_read(c, &totals[1], words + R, 8);
    if (e == hipSuccess) e = queue_read(c, &totals[2], bases + R, 8);
    if (e == hipSuccess) e = queue_read(c, h_stat, d_stat, sizeof h_stat);
    if (e == hipSuccess) e = rfxi::sync(c);  // the first wait: the totals the result is allocated by
    if (e != hipSuccess) return fail(e, "RFX_E_HIP", "");
  }
  const uint64_t S = totals[0], W = totals[1];
  if (S >= (1ull << 32) || W >= (1ull << 32)) return fail(hipSuccess, "RFX_E_RANGE", "the block would reach 2^32 reads or words");
  r->n = (uint32_t)S;
  r->n_words = W;
  r->n_bases = totals[2];
  r->max_len = h_stat[0];
  for (int l = 0; l < 32; ++l) r->short_cnt[l] = h_stat[1 + l];
  r->codes = (uint64_t*)dmalloc(c, std::max<uint64_t>(W, 1) * 8);
  r->good = (uint32_t*)dmalloc(c, std::max<uint64_t>(W, 1) * 4);
  r->word_off = (uint32_t*)dmalloc(c, ((size_t)S + 1) * 4);
  r->len = (uint32_t*)dmalloc(c, std::max<uint64_t>(S, 1) * 4);
  rec_at = (uint32_t*)dmalloc(c, std::max<uint64_t>(S, 1) * 4);
  ref_id = (int32_t*)dmalloc(c, std::max<uint64_t>(S, 1) * 4);
  run_rank = (uint64_t*)dmalloc(c, (S + 1) * 8);
  if (!r->codes || !r->good || !r->word_off || !r->len || !rec_at || !ref_id || !run_rank)
    return fail(hipSuccess, "RFX_E_NOMEM", "out of device memory");
  const uint32_t w_end = (uint32_t)W;
  uint64_t runs = 0;
  hipError_t e = hipMemcpyAsync(r->word_off + S, &w_end, 4, hipMemcpyHostToDevice, c->stream);  // (w_end lives until the wait below)
  if (e != hipSuccess) return fail(e, "RFX_E_HIP", "");
  if (S) {
    {
      rfx_span sp(c, "k_bamf_table");
      hipLaunchKernelGGL(k_bamf_table, grid_of(R, 16), dim3(256), 0, c->stream, arena, slot.rec_start, R, exclude_flags, (const uint8_t*)slot.region, cnt, words,
                         bases, r->len, r->word_off, rec_at, ref_id);
    }
    {
      rfx_span sp(c, "k_bam_runs");
      hipLaunchKernelGGL(k_bam_runs, grid_of(S, 16), dim3(256), 0, c->stream, ref_id, (uint32_t)S, run_rank);
    }
    rfxk::scan_tail(c, run_rank, S);
    e = queue_read(c, &runs, run_rank + S, 8);
    if (e != hipSuccess) return fail(e, "RFX_E_HIP", "");
    if (W) {
      rfx_span sp(c, "k_bamf_pack");
      hipLaunchKernelGGL(k_bamf_pack, grid_of(W, 32), dim3(256), 0, c->stream, arena, r->word_off, r->len, rec_at, (uint32_t)S, W, min_q,
                         r->codes, r->good);
    }
  }
  e = rfxi::sync(c);  // the second wait: the block is packed, the number of runs is known
  if (e != hipSuccess) return fail(e, "RFX_E_HIP", "");
  *n_runs = runs;
  if (runs > cap) return fail(hipSuccess, "RFX_E_RANGE", "more reference runs than the caller has room for");
  if (runs) {
    d_runs = (uint32_t*)dmalloc(c, runs * 8);
    if (!d_runs) return fail(hipSuccess, "RFX_E_NOMEM", "out of device memory");
    {
      rfx_span sp(c, "k_bam_run_out");
      hipLaunchKernelGGL(k_bam_run_out, grid_of(S, 16), dim3(256), 0, c->stream, ref_id, (uint32_t)S, run_rank, d_runs);
    }
    e = hipMemcpyAsync(ref_runs, d_runs, runs * 8, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = rfxi::sync(c);
    if (e != hipSuccess) return fail(e, "RFX_E_HIP", "");
  }
  dfree(c, cnt); dfree(c, words); dfree(c, bases); dfree(c, d_stat); dfree(c, rec_at); dfree(c, ref_id); dfree(c, run_rank);
  dfree(c, d_runs);
  return r;
}

int rfx_bam_name_hashes(rfx_text* t, uint32_t exclude_flags, const uint64_t* mask, uint64_t n_kept, uint64_t* out, uint64_t cap,
                        uint64_t* n_out) {
  static const char* const who = "rfx_bam_name_hashes";
  if (n_out) *n_out = 0;
  if (!t || !n_out || (cap && !out)) return RFX_E_INVAL;
  kept_view v;
  if (const int rc = kept_of(t, exclude_flags, who, &v)) return rc;
  rfx_ctx* c = v.c;
  if (v.n_kept != n_kept) {
    dfree(c, v.kept_at);
    return pull_fail(c, who, RFX_E_INVAL, hipSuccess, "n_kept is not the number of kept records of the arena");
  }
  const uint64_t nw = (n_kept + 63) / 64;
  const uint64_t tail = (n_kept & 63u) ? (1ull << (n_kept & 63u)) - 1ull : ~0ull;
  std::vector<uint64_t> h_mask, rank;  // the mask without the bits at and above n_kept; the selected in front of each word
  uint64_t n_sel = n_kept;
  if (mask) {
    h_mask.assign(mask, mask + nw);
    if (nw) h_mask[nw - 1] &= tail;
    rank.resize(nw);
    n_sel = 0;
    for (uint64_t w = 0; w < nw; ++w) {
      rank[w] = n_sel;
      n_sel += (uint64_t)__builtin_popcountll(h_mask[w]);
    }
  }
  *n_out = n_sel;
  if (n_sel > cap) {
    dfree(c, v.kept_at);
    return pull_fail(c, who, RFX_E_RANGE, hipSuccess, "the output buffer is too small");
  }
  if (n_sel == 0) {
    dfree(c, v.kept_at);
    return RFX_OK;
  }
  uint64_t* d_mask = mask ? (uint64_t*)dmalloc(c, (size_t)nw * 16) : nullptr;  // the mask, then the ranks
  uint64_t* d_out = (uint64_t*)dmalloc(c, (size_t)n_sel * 8);
  auto done = [&](int rc, hipError_t e, const char* text) {
    if (rc) pull_fail(c, who, rc, e, text);
    dfree(c, v.kept_at); dfree(c, d_mask); dfree(c, d_out);
    return rc;
  };
  if ((mask && !d_mask) || !d_out) return done(RFX_E_NOMEM, hipSuccess, "out of device memory");
  hipError_t e = hipSuccess;
  if (mask) {  // (pageable host memory: the runtime has copied it out when the call returns)
    e = hipMemcpyAsync(d_mask, h_mask.data(), (size_t)nw * 8, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d_mask + nw, rank.data(), (size_t)nw * 8, hipMemcpyHostToDevice, c->stream);
    if (e != hipSuccess) return done(RFX_E_HIP, e, "");
  }
  {
    rfx_span sp(c, "k_bam_hashes");
    const dim3 grid((unsigned)std::min<uint64_t>((n_kept + 255) / 256, (uint64_t)c->n_cu * 16));
    hipLaunchKernelGGL(k_bam_hashes, grid, dim3(256), 0, c->stream, v.arena, v.kept_at, n_kept, (const uint64_t*)d_mask,
                       (const uint64_t*)(d_mask ? d_mask + nw : nullptr), d_out);
  }
  e = hipMemcpyAsync(out, d_out, (size_t)n_sel * 8, hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = rfxi::sync(c);
  if (e != hipSuccess) return done(RFX_E_HIP, e, "");
  return done(RFX_OK, hipSuccess, "");
}

rfx_nameset* rfx_nameset_build(rfx_ctx* c, const uint64_t* hashes, uint64_t n) {
  if (!c || (n && !hashes)) {
    rfxi::set_error("rfx_nameset_build: RFX_E_INVAL: a NULL argument");
    return nullptr;
  }
  (void)hipSetDevice(c->device);
  uint64_t slots = 64;
  while (slots < 2 * n + 2) slots <<= 1;  // at most half full: a probe ends at an empty slot
  std::vector<uint64_t> table((size_t)slots, 0);
  rfx_nameset* s = new rfx_nameset{c, nullptr, slots, 0, 0};
  for (uint64_t i = 0; i < n; ++i) {
    const uint64_t key = hashes[i];
    if (key == 0) {
      s->n += !s->has_zero;
      s->has_zero = 1;
      continue;
    }
    uint64_t at = nameset_slot(key, slots);
    while (table[at] != 0 && table[at] != key) at = (at + 1) & (slots - 1);
    s->n += table[at] == 0;
    table[at] = key;
  }
  s->table = (uint64_t*)dmalloc(c, (size_t)slots * 8);
  hipError_t e = s->table ? hipMemcpyAsync(s->table, table.data(), (size_t)slots * 8, hipMemcpyHostToDevice, c->stream) : hipSuccess;
  if (s->table && e == hipSuccess) e = rfxi::sync(c);
  if (!s->table || e != hipSuccess) {
    pull_fail(c, "rfx_nameset_build", RFX_E_HIP, e, "RFX_E_NOMEM: out of device memory");
    dfree(c, s->table);
    delete s;
    return nullptr;
  }
  return s;
}
uint64_t rfx_nameset_size(const rfx_nameset* s) { return s ? s->n : 0; }
void rfx_nameset_free(rfx_nameset* s) {
  if (!s) return;
  dfree(s->ctx, s->table);
  delete s;
}

int rfx_bam_mark_names(rfx_text* t, uint32_t exclude_flags, const rfx_nameset* set, uint64_t* mask_out, uint64_t* n_kept,
                       uint64_t* n_marked) {
  static const char* const who = "rfx_bam_mark_names";
  if (n_kept) *n_kept = 0;
  if (n_marked) *n_marked = 0;
  if (!t || !set || !n_kept) return RFX_E_INVAL;
  if (rfxi::text_ctx(t) != set->ctx) return pull_fail(nullptr, who, RFX_E_INVAL, hipSuccess, "the set belongs to another context");
  kept_view v;
  if (const int rc = kept_of(t, exclude_flags, who, &v)) return rc;
  rfx_ctx* c = v.c;
  *n_kept = v.n_kept;
  if (v.n_kept == 0) return RFX_OK;
  if (!mask_out) {
    dfree(c, v.kept_at);
    return pull_fail(c, who, RFX_E_INVAL, hipSuccess, "mask_out is NULL");
  }
  const uint64_t nw = (v.n_kept + 63) / 64;
  uint64_t* d_mask = (uint64_t*)dmalloc(c, (size_t)(nw + 1) * 8);  // the mask, then the number of set bits
  auto done = [&](int rc, hipError_t e, const char* text) {
    if (rc) pull_fail(c, who, rc, e, text);
    dfree(c, v.kept_at); dfree(c, d_mask);
    return rc;
  };
  if (!d_mask) return done(RFX_E_NOMEM, hipSuccess, "out of device memory");
  hipError_t e = hipMemsetAsync(d_mask + nw, 0, 8, c->stream);
  if (e != hipSuccess) return done(RFX_E_HIP, e, "");
  {
    rfx_span sp(c, "k_bam_mark");
    const dim3 grid((unsigned)std::min<uint64_t>((nw + 3) / 4, (uint64_t)c->n_cu * 16));
    hipLaunchKernelGGL(k_bam_mark, grid, dim3(256), 0, c->stream, v.arena, v.kept_at, v.n_kept, (const uint64_t*)set->table, set->slots,
                       set->has_zero, d_mask, (unsigned long long*)(d_mask + nw));
  }
  uint64_t marked = 0;
  e = hipMemcpyAsync(mask_out, d_mask, (size_t)nw * 8, hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = queue_read(c, &marked, d_mask + nw, 8);
  if (e == hipSuccess) e = rfxi::sync(c);
  if (e != hipSuccess) return done(RFX_E_HIP, e, "");
  if (n_marked) *n_marked = marked;
  return done(RFX_OK, hipSuccess, "");
}

int rfx_bam_gather(rfx_text* t, uint32_t exclude_flags, const uint64_t* mask, uint64_t n_kept, void* host_out, uint64_t cap,
                   uint64_t* bytes_out, uint64_t* n_selected) {
  static const char* const who = "rfx_bam_gather";
  if (bytes_out) *bytes_out = 0;
  if (n_selected) *n_selected = 0;
  if (!t || !bytes_out || (n_kept && !mask) || (cap && !host_out)) return RFX_E_INVAL;
  kept_view v;
  if (const int rc = kept_of(t, exclude_flags, who, &v)) return rc;
  rfx_ctx* c = v.c;
  if (v.n_kept != n_kept) {
    dfree(c, v.kept_at);
    return pull_fail(c, who, RFX_E_INVAL, hipSuccess, "n_kept is not the number of kept records of the arena");
  }
  if (n_kept == 0) return RFX_OK;
  const uint32_t nw = (uint32_t)((n_kept + 63) / 64);
  const uint64_t tail = (n_kept & 63u) ? (1ull << (n_kept & 63u)) - 1ull : ~0ull;
  uint64_t* d_mask = (uint64_t*)dmalloc(c, (size_t)nw * 8);
  uint64_t* cnt = (uint64_t*)dmalloc(c, ((size_t)nw + 1) * 8);
  uint64_t* sizes = (uint64_t*)dmalloc(c, ((size_t)nw + 1) * 8);
  uint32_t *src_off = nullptr, *dst_off = nullptr, *out = nullptr;
  auto done = [&](int rc, hipError_t e, const char* text) {
    if (rc) pull_fail(c, who, rc, e, text);
    dfree(c, v.kept_at); dfree(c, d_mask); dfree(c, cnt); dfree(c, sizes); dfree(c, src_off); dfree(c, dst_off); dfree(c, out);
    return rc;
  };
  if (!d_mask || !cnt || !sizes) return done(RFX_E_NOMEM, hipSuccess, "out of device memory");
  const dim3 per_word((unsigned)std::min<uint64_t>(((uint64_t)nw + 255) / 256, (uint64_t)c->n_cu * 16));
  // the mask upload (pageable host memory: the runtime has copied it out of `mask` when the call returns)
  hipError_t e = hipMemcpyAsync(d_mask, mask, (size_t)nw * 8, hipMemcpyHostToDevice, c->stream);
  if (e != hipSuccess) return done(RFX_E_HIP, e, "");
  {
    rfx_span sp(c, "k_bamg_sizes");
    hipLaunchKernelGGL(k_bamg_sizes, per_word, dim3(256), 0, c->stream, v.arena, v.kept_at, d_mask, nw, tail, cnt, sizes);
  }
  rfxk::scan_tail(c, cnt, nw);
  rfxk::scan_tail(c, sizes, nw);
  uint64_t n_sel = 0, n_bytes = 0;
  e = queue_read(c, &n_sel, cnt + nw, 8);
  if (e == hipSuccess) e = queue_read(c, &n_bytes, sizes + nw, 8);
  if (e == hipSuccess) e = rfxi::sync(c);  // the one wait between the mask and the result: what the result is sized by
  if (e != hipSuccess) return done(RFX_E_HIP, e, "");
  *bytes_out = n_bytes;
  if (n_selected) *n_selected = n_sel;
  if (n_bytes > cap) return done(RFX_E_RANGE, hipSuccess, "the output buffer is too small");
  if (n_bytes == 0) return done(RFX_OK, hipSuccess, "");
  if (n_bytes > v.n) return done(RFX_E_HIP, hipSuccess, "the selection is larger than the arena");  // (cannot be: a subset)
  src_off = (uint32_t*)dmalloc(c, (size_t)n_sel * 4);
  dst_off = (uint32_t*)dmalloc(c, ((size_t)n_sel + 1) * 4);
  out = (uint32_t*)dmalloc(c, ((size_t)n_bytes + 3) / 4 * 4);
  if (!src_off || !dst_off || !out) return done(RFX_E_NOMEM, hipSuccess, "out of device memory");
  {
    rfx_span sp(c, "k_bamg_table");
    hipLaunchKernelGGL(k_bamg_table, per_word, dim3(256), 0, c->stream, v.arena, v.kept_at, d_mask, nw, tail, cnt, sizes, src_off, dst_off);
  }
  // (every source dword lies inside the arena or in the 8 KiB behind its capacity: k_gather_copy reads at most 7 bytes
  // behind a record's last byte, and a record lies in front of the arena's cut)
  rfxi::gather_copy(c, v.arena, src_off, dst_off, (uint32_t)n_sel, (uint32_t)n_bytes, out);
  e = hipGetLastError();
  if (e == hipSuccess) e = hipMemcpyAsync(host_out, out, (size_t)n_bytes, hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = rfxi::sync(c);
  if (e != hipSuccess) return done(RFX_E_HIP, e, "");
  return done(RFX_OK, hipSuccess, "");
}

// The single-end read pull (RUFUS.Filter.single --bam): see the section in front of k_bamh_pick.
int rfx_bam_gather_hits(rfx_text* t, uint32_t exclude_flags, rfx_set* set, const rfx_reads* block, int thresh, int last_base_skipped,
                        void* host_out, uint64_t cap, uint64_t* bytes_out, uint32_t* hits_out, uint32_t* index_out, uint64_t sel_cap,
                        uint64_t* n_selected) {
  static const char* const who = "rfx_bam_gather_hits";
  if (bytes_out) *bytes_out = 0;
  if (n_selected) *n_selected = 0;
  if (!t || !set || !block || !bytes_out || !n_selected || (cap && !host_out) || (sel_cap && !hits_out))
    return pull_fail(nullptr, who, RFX_E_INVAL, hipSuccess, "a NULL argument");
  if (rfxi::text_ctx(t) != set->ctx || block->ctx != set->ctx)
    return pull_fail(nullptr, who, RFX_E_INVAL, hipSuccess, "the arena, the set and the block belong to different contexts");
  if (!block->good) return pull_fail(nullptr, who, RFX_E_INVAL, hipSuccess, "the block is not a filter block (no quality mask)");
  kept_view v;
  if (const int rc = kept_of(t, exclude_flags, who, &v)) return rc;
  rfx_ctx* c = v.c;
  if (v.n_kept != block->n) {
    dfree(c, v.kept_at);
    return pull_fail(c, who, RFX_E_INVAL, hipSuccess, "the block does not hold the kept records of the arena as it is now");
  }
  if (v.n_kept == 0) return RFX_OK;
  const uint64_t nw = (v.n_kept + 63) / 64;
  uint64_t* cnt = (uint64_t*)dmalloc(c, ((size_t)nw + 1) * 8);
  uint64_t* sizes = (uint64_t*)dmalloc(c, ((size_t)nw + 1) * 8);
  uint32_t *src_off = nullptr, *dst_off = nullptr, *hits_sel = nullptr, *index_sel = nullptr, *out = nullptr;
  std::vector<void*> held;  // the filter's buffers: the counts among them
  auto done = [&](int rc, hipError_t e, const char* text) {
    if (rc) pull_fail(c, who, rc, e, text);  // (waits: a read-back into a local below may be queued)
    dfree(c, v.kept_at); dfree(c, cnt); dfree(c, sizes); dfree(c, src_off); dfree(c, dst_off); dfree(c, hits_sel); dfree(c, index_sel);
    dfree(c, out);
    for (void* p : held) dfree(c, p);
    return rc;
  };
  if (!cnt || !sizes) return done(RFX_E_NOMEM, hipSuccess, "out of device memory");
  unsigned long long nh = 0;
  uint64_t n_sel = 0, n_bytes = 0;
  const uint32_t* d_hits = nullptr;
  if (const int rc = rfxi::filter_counts_queue(set, block, thresh, last_base_skipped, &nh, held, &d_hits))
    return done(rc, hipSuccess, rc == RFX_E_NOMEM ? "out of device memory" : "the filter could not be queued");
  const dim3 per_wave((unsigned)std::min<uint64_t>((nw + 3) / 4, (uint64_t)c->n_cu * 16));
  {
    rfx_span sp(c, "k_bamh_pick");
    hipLaunchKernelGGL(k_bamh_pick, per_wave, dim3(256), 0, c->stream, v.arena, v.kept_at, d_hits, v.n_kept, thresh, cnt, sizes);
  }
  rfxk::scan_tail(c, cnt, nw);
  rfxk::scan_tail(c, sizes, nw);
  hipError_t e = queue_read(c, &n_sel, cnt + nw, 8);
  if (e == hipSuccess) e = queue_read(c, &n_bytes, sizes + nw, 8);
  if (e == hipSuccess) e = rfxi::sync(c);  // the first wait: what the result is sized by
  if (e != hipSuccess) return done(RFX_E_HIP, e, "");
  *bytes_out = n_bytes;
  *n_selected = n_sel;
  if (n_bytes > cap || n_sel > sel_cap) return done(RFX_E_RANGE, hipSuccess, "an output buffer is too small");
  if (n_sel == 0) return done(RFX_OK, hipSuccess, "");
  if (n_bytes > v.n) return done(RFX_E_HIP, hipSuccess, "the selection is larger than the arena");  // (cannot be: a subset)
  src_off = (uint32_t*)dmalloc(c, (size_t)n_sel * 4);
  dst_off = (uint32_t*)dmalloc(c, ((size_t)n_sel + 1) * 4);
  hits_sel = (uint32_t*)dmalloc(c, (size_t)n_sel * 4);
  index_sel = (uint32_t*)dmalloc(c, (size_t)n_sel * 4);
  out = (uint32_t*)dmalloc(c, ((size_t)n_bytes + 3) / 4 * 4);
  if (!src_off || !dst_off || !hits_sel || !index_sel || !out) return done(RFX_E_NOMEM, hipSuccess, "out of device memory");
  {
    rfx_span sp(c, "k_bamh_table");
    hipLaunchKernelGGL(k_bamh_table, per_wave, dim3(256), 0, c->stream, v.arena, v.kept_at, d_hits, v.n_kept, thresh, cnt, sizes, src_off,
                       dst_off, hits_sel, index_sel);
  }
  // (the sources are whole records of the arena, as in rfx_bam_gather)
  rfxi::gather_copy(c, v.arena, src_off, dst_off, (uint32_t)n_sel, (uint32_t)n_bytes, out);
  e = hipGetLastError();
  if (e == hipSuccess) e = hipMemcpyAsync(host_out, out, (size_t)n_bytes, hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(hits_out, hits_sel, (size_t)n_sel * 4, hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess && index_out) e = hipMemcpyAsync(index_out, index_sel, (size_t)n_sel * 4, hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = rfxi::sync(c);  // the second wait: the result is in the caller's memory
  if (e != hipSuccess) return done(RFX_E_HIP, e, "");
  return done(RFX_OK, hipSuccess, "");
}


// ---- a record's address, and records fetched by address (count --bam --keep-packed, RUFUS.Filter --packed) ---------------
// Replaces the second and third inflate of the subject's BAM (scripts/RunJellyForRUFUS.sh:28-29, then the two passes of
// runRufus.sh:964-967): the count notes where every kept record lies, the filter asks for the hit names' records alone.
//
//   k_bam_locate     a thread per kept record (kept_of's rank): its arena offset and 4 + block_size
//   k_fetch_check    a thread per list entry: the three checks, the lowest failing index (atomicMin), bytes[] widened -> a scan
//   k_fetch_table    a thread per entry of a run: source offset, destination offset inside the run   -> k_gather_copy
//   k_nameset_mark   k_bam_mark with the hash taken from an array: a lane per hash, the ballot = the mask word
int rfx_bam_locate(rfx_text* t, uint32_t exclude_flags, uint64_t n_kept, uint32_t* start_out, uint32_t* bytes_out) {
  static const char* const who = "rfx_bam_locate";
  if (!t || (n_kept && (!start_out || !bytes_out))) return RFX_E_INVAL;
  kept_view v;
  if (const int rc = kept_of(t, exclude_flags, who, &v)) return rc;
  rfx_ctx* c = v.c;
  if (v.n_kept != n_kept) {
    dfree(c, v.kept_at);
    return pull_fail(c, who, RFX_E_INVAL, hipSuccess, "n_kept is not the number of kept records of the arena");
  }
  if (n_kept == 0) return RFX_OK;
  uint32_t* d_out = (uint32_t*)dmalloc(c, (size_t)n_kept * 8);  // the starts, then the sizes
  auto done = [&](int rc, hipError_t e, const char* text) {
    if (rc) pull_fail(c, who, rc, e, text);
    dfree(c, v.kept_at); dfree(c, d_out);
    return rc;
  };
  if (!d_out) return done(RFX_E_NOMEM, hipSuccess, "out of device memory");
  {
    rfx_span sp(c, "k_bam_locate");
    const dim3 grid((unsigned)std::min<uint64_t>((n_kept + 255) / 256, (uint64_t)c->n_cu * 16));
    hipLaunchKernelGGL(k_bam_locate, grid, dim3(256), 0, c->stream, v.arena, (const uint32_t*)v.kept_at, n_kept, d_out, d_out + n_kept);
  }
  hipError_t e = hipMemcpyAsync(start_out, d_out, (size_t)n_kept * 4, hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(bytes_out, d_out + n_kept, (size_t)n_kept * 4, hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = rfxi::sync(c);
  if (e != hipSuccess) return done(RFX_E_HIP, e, "");
  return done(RFX_OK, hipSuccess, "");
}

int rfx_bam_fetch(rfx_text* t, const uint32_t* start, const uint32_t* bytes, uint64_t n, void* host_out, uint64_t cap,
                  uint64_t* out_bytes) {
  static const char* const who = "rfx_bam_fetch";
  if (out_bytes) *out_bytes = 0;
  if (!t || !out_bytes || (n && (!start || !bytes)) || (cap && !host_out)) return RFX_E_INVAL;
  rfx_ctx* c = nullptr;
  const uint8_t* arena = nullptr;
  uint64_t used = 0;
  if (const int rc = rfxi::text_ready(t, &c, &arena, &used)) return rc;  // waits for the appends; a block that did not inflate
  if (n == 0) return RFX_OK;
  if (n >= BAM_NONE) return pull_fail(c, who, RFX_E_RANGE, hipSuccess, "2^32 - 1 entries or more");
  uint32_t* d_list = (uint32_t*)dmalloc(c, (size_t)n * 8 + 4);  // start, bytes, the lowest failing index
  uint64_t* sizes = (uint64_t*)dmalloc(c, ((size_t)n + 1) * 8);
  uint32_t *src_off = nullptr, *dst_off = nullptr, *out = nullptr;
  auto done = [&](int rc, hipError_t e, const char* text) {
    if (rc) pull_fail(c, who, rc, e, text);
    dfree(c, d_list); dfree(c, sizes); dfree(c, src_off); dfree(c, dst_off); dfree(c, out);
    return rc;
  };
  if (!d_list || !sizes) return done(RFX_E_NOMEM, hipSuccess, "out of device memory");
  uint32_t *d_start = d_list, *d_bytes = d_list + n, *d_bad = d_list + 2 * n;
  const dim3 per_entry((unsigned)std::min<uint64_t>((n + 255) / 256, (uint64_t)c->n_cu * 16));
  // (pageable host memory: the runtime has copied it out of the lists when the call returns)
  hipError_t e = hipMemcpyAsync(d_start, start, (size_t)n * 4, hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(d_bytes, bytes, (size_t)n * 4, hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) e = hipMemsetAsync(d_bad, 0xFF, 4, c->stream);
  if (e != hipSuccess) return done(RFX_E_HIP, e, "");
  {
    rfx_span sp(c, "k_fetch_check");
    hipLaunchKernelGGL(k_fetch_check, per_entry, dim3(256), 0, c->stream, arena, used, (const uint32_t*)d_start,
                       (const uint32_t*)d_bytes, n, d_bad, sizes);
  }
  rfxk::scan_tail(c, sizes, n);
  uint32_t bad = BAM_NONE;
  uint64_t total = 0;
  e = queue_read(c, &bad, d_bad, 4);
  if (e == hipSuccess) e = queue_read(c, &total, sizes + n, 8);
  if (e == hipSuccess) e = rfxi::sync(c);  // the one wait between the lists and the copy: the verdict and the size
  if (e != hipSuccess) return done(RFX_E_HIP, e, "");
  if (bad != BAM_NONE) {
    char msg[200];
    snprintf(msg, sizeof msg, "entry %u (start %u, bytes %u) is not a record inside the arena's %llu bytes", bad, start[bad], bytes[bad],
             (unsigned long long)used);
    return done(RFX_E_FORMAT, hipSuccess, msg);
  }
  *out_bytes = total;
  if (total > cap) return done(RFX_E_RANGE, hipSuccess, "the output buffer is too small");
  // Runs of the list, each one k_gather_copy: a run ends in front of an entry that starts in the arena's first four bytes
  // (the kernel reads the dword a record shares with its predecessor from `have` bytes in front of the record: a record
  // that follows another must not lie there) and where it would pass 1 GiB (the kernel's offsets are 32 bits).  A list the
  // tool makes -- ascending, out of blocks that begin with other bytes -- is one run.
  constexpr uint64_t RUN_MAX = 1ull << 30;
  std::vector<uint64_t> run_first, run_at;  // the run's first entry, its first byte in the result
  uint64_t at = 0, run_bytes = 0, longest = 0, most = 0;
  for (uint64_t i = 0; i < n; ++i) {
    if (i == 0 || start[i] < 4u || run_bytes + bytes[i] > RUN_MAX) {
      run_first.push_back(i);
      run_at.push_back(at);
      run_bytes = 0;
    }
    run_bytes += bytes[i];
    at += bytes[i];
    longest = std::max(longest, run_bytes);
    most = std::max(most, i + 1 - run_first.back());
  }
  if (at != total) return done(RFX_E_HIP, hipSuccess, "the device's total differs from the host's");  // (cannot be)
  src_off = (uint32_t*)dmalloc(c, (size_t)most * 4);
  dst_off = (uint32_t*)dmalloc(c, ((size_t)most + 1) * 4);
  out = (uint32_t*)dmalloc(c, ((size_t)longest + 3) / 4 * 4);
  if (!src_off || !dst_off || !out) return done(RFX_E_NOMEM, hipSuccess, "out of device memory");
  run_first.push_back(n);
  run_at.push_back(total);
  for (size_t r = 0; r + 1 < run_first.size(); ++r) {  // (the buffers are reused in stream order)
    const uint64_t first = run_first[r], m = run_first[r + 1] - first, nb = run_at[r + 1] - run_at[r];
    {
      rfx_span sp(c, "k_fetch_table");
      const dim3 grid((unsigned)std::min<uint64_t>((m + 255) / 256, (uint64_t)c->n_cu * 16));
      hipLaunchKernelGGL(k_fetch_table, grid, dim3(256), 0, c->stream, (const uint32_t*)d_start + first, (const uint64_t*)sizes + first,
                         (uint32_t)m, src_off, dst_off);
    }
    // (every source dword lies inside the arena or in the 8 KiB behind its capacity: k_gather_copy reads at most 7 bytes
    // behind a record's last byte, and the check has put every record in front of the arena's end)
    rfxi::gather_copy(c, arena, src_off, dst_off, (uint32_t)m, (uint32_t)nb, out);
    e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync((uint8_t*)host_out + run_at[r], out, (size_t)nb, hipMemcpyDeviceToHost, c->stream);
    if (e != hipSuccess) return done(RFX_E_HIP, e, "");
  }
  e = rfxi::sync(c);
  if (e != hipSuccess) return done(RFX_E_HIP, e, "");
  return done(RFX_OK, hipSuccess, "");
}

int rfx_nameset_mark(const rfx_nameset* set, const uint64_t* hashes, uint64_t n, uint64_t* mask_out, uint64_t* n_marked) {
  static const char* const who = "rfx_nameset_mark";
  if (n_marked) *n_marked = 0;
  if (!set || (n && (!hashes || !mask_out))) return RFX_E_INVAL;
  if (n == 0) return RFX_OK;
  rfx_ctx* c = set->ctx;
  (void)hipSetDevice(c->device);
  uint64_t piece = 1ull << 22;  // hashes per upload: 32 MiB, whatever n is (RFX_NAMESET_PIECE: a test knob, changes no result)
  if (const char* env = getenv("RFX_NAMESET_PIECE")) {
    const long long want = atoll(env);
    if (want >= 64 && want <= (1ll << 26)) piece = (uint64_t)want & ~63ull;
  }
  piece = std::min<uint64_t>(piece, (n + 63) & ~63ull);
  const uint64_t n_pieces = (n + piece - 1) / piece;
  uint64_t* d_hash = (uint64_t*)dmalloc(c, (size_t)piece * 8);
  uint64_t* d_mask = (uint64_t*)dmalloc(c, (size_t)piece / 8);
  uint32_t* d_cnt = (uint32_t*)dmalloc(c, (size_t)n_pieces * 4);  // a piece's set bits: below 2^32, a 32-bit atomic each
  std::vector<uint32_t> cnt((size_t)n_pieces, 0);
  auto done = [&](int rc, hipError_t e, const char* text) {
    if (rc) pull_fail(c, who, rc, e, text);
    dfree(c, d_hash); dfree(c, d_mask); dfree(c, d_cnt);
    return rc;
  };
  if (!d_hash || !d_mask || !d_cnt) return done(RFX_E_NOMEM, hipSuccess, "out of device memory");
  hipError_t e = hipMemsetAsync(d_cnt, 0, (size_t)n_pieces * 4, c->stream);
  for (uint64_t p = 0; p < n_pieces && e == hipSuccess; ++p) {  // (the two buffers are reused in stream order)
    const uint64_t first = p * piece, m = std::min(piece, n - first), nw = (m + 63) / 64;
    e = hipMemcpyAsync(d_hash, hashes + first, (size_t)m * 8, hipMemcpyHostToDevice, c->stream);
    if (e != hipSuccess) break;
    {
      rfx_span sp(c, "k_nameset_mark");
      const dim3 grid((unsigned)std::min<uint64_t>((nw + 3) / 4, (uint64_t)c->n_cu * 16));
      hipLaunchKernelGGL(k_nameset_mark, grid, dim3(256), 0, c->stream, (const uint64_t*)d_hash, m, (const uint64_t*)set->table,
                         set->slots, set->has_zero, d_mask, d_cnt + p);
    }
    e = hipMemcpyAsync(mask_out + first / 64, d_mask, (size_t)nw * 8, hipMemcpyDeviceToHost, c->stream);
  }
  if (e == hipSuccess) e = hipMemcpyAsync(cnt.data(), d_cnt, (size_t)n_pieces * 4, hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = rfxi::sync(c);
  if (e != hipSuccess) return done(RFX_E_HIP, e, "");
  uint64_t marked = 0;
  for (const uint32_t x : cnt) marked += x;
  if (n_marked) *n_marked = marked;
  return done(RFX_OK, hipSuccess, "");
}

}  // extern "C"
