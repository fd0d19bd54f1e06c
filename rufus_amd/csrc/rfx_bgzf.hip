// k_bgzf_inflate: BGZF blocks inflated on the device, straight into the text arena of K1 (rfx_text.hip).  Replaces the
// host inflater of `zcat F.fastq.gz | ...` (runRufus.sh:157-160): one host thread there, one WAVEFRONT per BGZF block here.
//
// Why a wave per block.  A deflate stream is serial -- the position of every code depends on the codes before it -- but
// BGZF cuts a file into independent streams of <= 64 KiB, 16 K of them per GiB of text: the parallelism is across blocks.
// A thread per block would leave 63 of 64 lanes idle and scatter single bytes; a wave per block keeps the serial part
// (bit buffer, symbol decode: rfx_bgzf_core.h, the same statements the host harness runs under the sanitizers) uniform
// across the wave -- every lane computes the same values from the same addresses, so the compiler may keep them in
// scalar registers -- and gives the byte moving to the 64 lanes together: a run of literals (collected one per lane, then
// ONE store instruction), a match (byte i comes from out[pos - d + i % d], which always lies before pos, so an
// overlapping match, d = 1 included, needs no serial loop), a stored run, and afterwards the CRC-32 (each lane a slice,
// combined with the shift of rfx_bgzf_core.h).
//
// LDS budget: one bgzf_tables per wave = 4160 bytes (two fast tables of 1024 + 512 halfwords, the symbol lists, the counts,
// 320 code lengths).  A CU holds at most 32 waves: 32 x 4160 B = 130 KB of its 160 KB, so occupancy is bounded by waves,
// not by LDS.
//
// Lockstep.  The table builds of rfx_bgzf_core.h run on all 64 lanes at once, every lane storing the same value to the same
// LDS word, read-modify-writes included.  That is right because the workgroup is ONE wave64 (`__launch_bounds__(64)`,
// launched with 64 threads) in uniform control flow: the lanes execute each LDS instruction together, so all of them read
// the old word before the new one is stored.  A wider workgroup or lane-dependent control flow in the core would break it.
//
// Ordering.  A match LOADS bytes that earlier tokens' stores -- of other lanes -- wrote.  __syncthreads() (the workgroup
// is one wave: it costs next to nothing and its meaning is defined) stands between them; it is skipped when the match's
// source lies wholly below the position of the last synchronisation (`synced`), which is the common case in FASTQ text
// (matches reach back a record or more).  Nothing is ever stored twice, so there is no write-after-read hazard.
//
// Bounds.  The core calls the policy only with pos + len <= ISIZE and dist <= pos; the policy adds the block's output
// offset and nothing else, so no byte outside [out, out + ISIZE) of a block is read or written whatever the input says.
// The host (rfx_text_append_bgzf) checks that these ranges lie inside the arena before the launch.  Input is read only
// inside [payload, payload + size).  A failing block writes its status and the wave goes on to its next block.
#include "rfx_bgzf_core.h"
#include "rfx_internal.h"

namespace {

struct wave_out {
  uint8_t* out;
  uint32_t lane;
  uint32_t n_lit, lit_pos, lit;  // the literal run being collected: n_lit bytes from lit_pos on, lane i holds byte i
  uint32_t synced;               // every store to out[0, synced) is visible to all lanes

  __device__ __forceinline__ void flush() {
    if (lane < n_lit) out[lit_pos + lane] = (uint8_t)lit;
    n_lit = 0;
  }
  __device__ __forceinline__ void literal(uint32_t pos, uint32_t byte) {
    if (n_lit == 0) lit_pos = pos;
    if (lane == n_lit) lit = byte;
    if (++n_lit == 64u) flush();
  }
  __device__ __forceinline__ void match(uint32_t pos, uint32_t len, uint32_t dist) {
    flush();
    const uint32_t src = pos - dist, src_end = src + (len < dist ? len : dist);
    if (src_end > synced) {  // (wave-uniform: every lane of the one-wave workgroup arrives)
      __syncthreads();
      synced = pos;
    }
    for (uint32_t i = lane; i < len; i += 64u) out[pos + i] = out[src + (i < dist ? i : i % dist)];
  }
  __device__ __forceinline__ void stored(uint32_t pos, const uint8_t* from, uint32_t n) {
    flush();
    for (uint32_t i = lane; i < n; i += 64u) out[pos + i] = from[i];
  }
  __device__ __forceinline__ void end() { flush(); }
};

__global__ __launch_bounds__(64) void k_bgzf_inflate(const uint8_t* __restrict__ stage, const bgzf_desc* __restrict__ desc,
                                                      uint32_t n_blocks, uint32_t first_index, uint8_t* arena,
                                                      uint32_t* __restrict__ status, uint32_t* __restrict__ first_bad) {
  __shared__ bgzf_tables tables;
  const uint32_t lane = threadIdx.x;
  for (uint32_t blk = blockIdx.x; blk < n_blocks; blk += gridDim.x) {
    const bgzf_desc d = desc[blk];
    const uint8_t* in = stage + d.in_off;
    uint8_t* out = arena + d.out_off;
    wave_out wo{out, lane, 0u, 0u, 0u, 0u};
    uint32_t st = bgzf_inflate(in, in + d.in_len, d.isize, tables, wo);
    __syncthreads();  // the block's bytes are visible to every lane; the tables are free for the next block
    if (st == BGZF_OK) {
      uint32_t x = bgzf_crc_lane(out, d.isize, lane);
#pragma unroll
      for (int o = 32; o; o >>= 1) x ^= __shfl_xor(x, o);
      if (~x != d.crc) st = BGZF_E_CRC;
    }
    if (lane == 0) {
      status[blk] = st;
      if (st != BGZF_OK) atomicMin(first_bad, first_index + blk);
    }
  }
}

}  // namespace

namespace rfxk {

void bgzf_inflate(rfx_ctx* c, hipStream_t stream, const uint8_t* stage, const bgzf_desc* desc, uint32_t n_blocks,
                  uint32_t first_index, uint8_t* arena, uint32_t* status, uint32_t* first_bad) {
  if (!n_blocks) return;
  // a workgroup per block while that is a sane grid: blocks take unequal time (their compressed size), and the
  // dispatcher hands the next one to whichever wave slot is free; beyond it the grid-stride loop takes over
  const uint32_t grid = std::min<uint32_t>(n_blocks, (uint32_t)c->n_cu * 32u * 16u);
  hipLaunchKernelGGL(k_bgzf_inflate, dim3(grid), dim3(64), 0, stream, stage, desc, n_blocks, first_index, arena, status, first_bad);
}

}  // namespace rfxk
