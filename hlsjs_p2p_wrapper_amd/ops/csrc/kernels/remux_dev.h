// What remux.hip and mpeg_audio.hip share on the device: the workgroup geometry of the two remux
// kernels, the 64-bit workgroup scan of the plan, and the output-driven copy of one payload inside
// one 16 KiB tile (docs/REMUX.md, docs/MPEGAUDIO.md).
#pragma once
#include "es_dev.h"

namespace hlsp2p {
namespace dev {

constexpr int kRxThreads = 256;
constexpr int kRxWaves = kRxThreads / 64;
constexpr int kRxIterBytes = kRxThreads * 16;
constexpr int kRxIters = es::kRemuxTile / kRxIterBytes;
static_assert(kRxIters * kRxIterBytes == es::kRemuxTile, "the tile is a whole number of iterations");

// Exclusive prefix sum of 64-bit values over the workgroup (every thread calls it); total: the sum
// of all.  The wave step is a shuffle ladder (DPP moves 32 bits), the rest common.h wg_exclusive_prefix.
__device__ __forceinline__ int64_t rx_block_scan(int64_t v, int64_t* s_w, int64_t& total) {
  const int lane = threadIdx.x & 63;
  int64_t inc = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int64_t t = __shfl_up(inc, d);
    if (lane >= d) inc += t;
  }
  const WgPrefix<int64_t> p = wg_exclusive_prefix<kRxWaves>(inc, v, s_w);
  total = p.total;
  __syncthreads();  // s_w is free again
  return p.before;
}

__device__ __forceinline__ int32_t rx_sat32(int64_t v) { return v < 0x7fffffff ? static_cast<int32_t>(v) : 0x7fffffff; }

// last j in [lo, hi] with t[j] <= y, given t[lo] <= y (t ascends)
__device__ __forceinline__ int rx_last_le(const int32_t* __restrict__ t, int lo, int hi, int y) {
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (t[mid] <= y) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// One payload inside one tile.  Output bytes [lo, hi) of the region hold the payload: row j of
// `cnt` rows starts at payload offset start[j] (start[0] == 0, start[cnt] >= hi - lo) with kPrefix
// bytes of big-endian length, then the bytes of the segment's ES from src[j] on.  Every thread
// of the workgroup calls it.  The loads of the four iterations are issued together, phase by
// phase (rows, then source dwords), so a lane waits for two round trips, not eight.
template <int kPrefix>
__device__ __forceinline__ void rx_copy_stream(__amdgpu_buffer_rsrc_t rsrc, const uint8_t* __restrict__ V,
                                               uint8_t* __restrict__ o, int b0, int lo, int hi,
                                               const int32_t* __restrict__ start, const int32_t* __restrict__ src,
                                               int cnt) {
  const int t_lo = lo > b0 ? lo : b0;
  const int t_hi = hi < b0 + es::kRemuxTile ? hi : b0 + es::kRemuxTile;
  if (t_lo >= t_hi || cnt <= 0) return;  // workgroup-uniform
  const int j_lo = last_le_wave<int32_t>(start, cnt, t_lo - lo);  // workgroup-uniform: the rows this tile touches
  const int j_hi = last_le_wave<int32_t>(start, cnt, t_hi - 1 - lo);
  int c_lo[kRxIters], c_hi[kRxIters], j[kRxIters], e[kRxIters], nxt[kRxIters], sj[kRxIters];
#pragma unroll
  for (int it = 0; it < kRxIters; ++it) {
    const int x0 = b0 + it * kRxIterBytes + static_cast<int>(threadIdx.x) * 16;
    c_lo[it] = x0 > t_lo ? x0 : t_lo;
    c_hi[it] = x0 + 16 < t_hi ? x0 + 16 : t_hi;
    j[it] = c_lo[it] < c_hi[it] ? rx_last_le(start, j_lo, j_hi, c_lo[it] - lo) : j_lo;
  }
#pragma unroll
  for (int it = 0; it < kRxIters; ++it) {  // rows in range also for idle lanes: unconditional loads
    e[it] = start[j[it]];
    nxt[it] = start[j[it] + 1];
    sj[it] = src[j[it]];
  }
  bool fast[kRxIters];
  v4u v[kRxIters];
  uint32_t w4[kRxIters];
  int sa[kRxIters];
#pragma unroll
  for (int it = 0; it < kRxIters; ++it) {
    const int y = c_lo[it] - lo;
    fast[it] = c_hi[it] - c_lo[it] == 16 && y >= e[it] + kPrefix && y + 16 <= nxt[it];
    sa[it] = fast[it] ? sj[it] + (y - e[it] - kPrefix) : 0;
    v[it] = __builtin_amdgcn_raw_buffer_load_b128(rsrc, sa[it] & ~3, 0, 0);
    w4[it] = __builtin_amdgcn_raw_buffer_load_b32(rsrc, (sa[it] & ~3) + 16, 0, 0);
  }
#pragma unroll
  for (int it = 0; it < kRxIters; ++it) {
    if (fast[it]) {
      *reinterpret_cast<v4u*>(o + c_lo[it]) = funnel16(v[it], w4[it], static_cast<uint32_t>(sa[it] & 3));
      continue;
    }
    int jj = j[it];
    int y = c_lo[it] - lo;
    for (int x = c_lo[it]; x < c_hi[it]; ++x, ++y) {
      while (jj + 1 < cnt && start[jj + 1] <= y) ++jj;
      const int r = y - start[jj];
      uint8_t byte;
      if (r < kPrefix) {
        const uint32_t len = static_cast<uint32_t>(start[jj + 1] - start[jj] - kPrefix);
        byte = static_cast<uint8_t>(len >> (8 * (3 - r)));
      } else {
        byte = V[src[jj] + r - kPrefix];
      }
      o[x] = byte;
    }
  }
}

}  // namespace dev
}  // namespace hlsp2p
