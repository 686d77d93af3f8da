// Shared device helpers for the CDNA4 (gfx950) kernels.  Wave64 everywhere.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace hlsp2p {
namespace dev {

// Monotone segment walk: first index s with prefix[s + 1] > v, starting from `s`.
__device__ __forceinline__ int advance_seg(const int64_t* __restrict__ prefix, int s, int64_t v) {
  while (prefix[s + 1] <= v) ++s;
  return s;
}

// Largest j in [0, n) with t[j] <= v (t ascends, t[0] <= v) for a wave-uniform v, with all 64
// lanes active: each lane tests one row and a ballot counts the rows <= v, so the lookup costs
// ONE global round trip per 64-way level (n <= 64: one, n <= 4096: two) instead of log2(n)
// dependent loads at the head of every workgroup.
template <typename T>
__device__ __forceinline__ int last_le_wave(const T* __restrict__ t, int n, T v) {
  const int lane = static_cast<int>(threadIdx.x & 63);
  int lo = 0, cnt = n;  // answer in [lo, lo + cnt)
  while (cnt > 64) {
    const int stride = (cnt + 63) >> 6;
    const int idx = lo + lane * stride;
    const bool le = idx < lo + cnt && t[idx] <= v;
    lo += (__popcll(__ballot(le)) - 1) * stride;
    cnt = stride < n - lo ? stride : n - lo;
  }
  const bool le = lane < cnt && t[lo + lane] <= v;
  return __builtin_amdgcn_readfirstlane(lo + __popcll(__ballot(le)) - 1);
}
// The segment of tile (block, chunk) v: prefix has n + 1 ascending entries.
__device__ __forceinline__ int find_seg_wave(const int64_t* __restrict__ prefix, int n, int64_t v) {
  return last_le_wave(prefix, n, v);
}

// Inclusive prefix sum over the wave64 in six DPP-modified moves and adds, no LDS traffic
// (a __shfl_up ladder is six ds_bpermute round trips): row_shr:1/2/4/8 scan each 16-lane row
// (bound_ctrl fills 0 past the row start), row_bcast:15 adds row 0's / row 2's total to rows 1
// and 3, row_bcast:31 adds rows 0-1's total to rows 2 and 3.
__device__ __forceinline__ uint32_t wave_scan_dpp(uint32_t v) {
  v += static_cast<uint32_t>(__builtin_amdgcn_update_dpp(0, static_cast<int>(v), 0x111, 0xf, 0xf, true));
  v += static_cast<uint32_t>(__builtin_amdgcn_update_dpp(0, static_cast<int>(v), 0x112, 0xf, 0xf, true));
  v += static_cast<uint32_t>(__builtin_amdgcn_update_dpp(0, static_cast<int>(v), 0x114, 0xf, 0xf, true));
  v += static_cast<uint32_t>(__builtin_amdgcn_update_dpp(0, static_cast<int>(v), 0x118, 0xf, 0xf, true));
  v += static_cast<uint32_t>(__builtin_amdgcn_update_dpp(0, static_cast<int>(v), 0x142, 0xa, 0xf, false));
  v += static_cast<uint32_t>(__builtin_amdgcn_update_dpp(0, static_cast<int>(v), 0x143, 0xc, 0xf, false));
  return v;
}

// Exclusive prefix over a workgroup, called by every one of its 64 * kWaves threads (blockDim.x is
// exactly that, all lanes active): `inc` is the caller's inclusive scan of `own` inside the wave
// (DPP, ballot / popcount or shuffles).  Lane 63 leaves the wave's total in s_wave, kWaves words
// of LDS; one barrier stands between that store and the reads.  The barrier that frees s_wave for
// the next call is the caller's.
template <typename T>
struct WgPrefix {
  T before, total;  // the sum of `own` over the threads in front of this one, and over all
};
template <int kWaves, typename T>
__device__ __forceinline__ WgPrefix<T> wg_exclusive_prefix(T inc, T own, T* s_wave) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 63) s_wave[wave] = inc;
  __syncthreads();
  WgPrefix<T> p = {inc - own, 0};
#pragma unroll
  for (int w = 0; w < kWaves; ++w) {
    if (w < wave) p.before += s_wave[w];
    p.total += s_wave[w];
  }
  return p;
}

typedef unsigned int v4u __attribute__((ext_vector_type(4)));
typedef int v4i __attribute__((ext_vector_type(4)));

// Bytes [sh, sh + 16) of the five dwords v.x v.y v.z v.w w4, sh in 0..3: four v_alignbyte.
__device__ __forceinline__ v4u funnel16(v4u v, uint32_t w4, uint32_t sh) {
  return v4u{__builtin_amdgcn_alignbyte(v.y, v.x, sh), __builtin_amdgcn_alignbyte(v.z, v.y, sh),
             __builtin_amdgcn_alignbyte(v.w, v.z, sh), __builtin_amdgcn_alignbyte(w4, v.w, sh)};
}
// 16 bytes at any byte offset of a buffer resource: the five dwords around them, funnelled; a
// dword beyond the resource's range reads as zero.
__device__ __forceinline__ v4u load16_unaligned(__amdgpu_buffer_rsrc_t rsrc, int off) {
  const v4u v = __builtin_amdgcn_raw_buffer_load_b128(rsrc, off & ~3, 0, 0);
  const uint32_t w4 = __builtin_amdgcn_raw_buffer_load_b32(rsrc, (off & ~3) + 16, 0, 0);
  return funnel16(v, w4, static_cast<uint32_t>(off & 3));
}

// Workgroup copy of `count` elements global -> LDS with every load of the thread issued
// before its first LDS store (kIters >= ceil(count / nthreads)).  The plain strided loop
// compiles to load / s_waitcnt vmcnt(0) / ds_write per element: one L2 round trip per
// iteration, serialised — 8-40 of them at the head of a kernel.
template <int kIters, typename T>
__device__ __forceinline__ void lds_fill(T* __restrict__ dst, const T* __restrict__ src, int count, int tid,
                                         int nthreads) {
  T v[kIters];
  const int last = count - 1;
#pragma unroll
  for (int k = 0; k < kIters; ++k) {
    const int i = tid + k * nthreads;
    v[k] = src[i < last ? i : last];
  }
  // out-of-range lanes store src[last] to dst[last] again (same value): an unconditional
  // store keeps the compiler from sinking each load into a guarded block next to its store
#pragma unroll
  for (int k = 0; k < kIters; ++k) {
    const int i = tid + k * nthreads;
    dst[i < last ? i : last] = v[k];
  }
}

}  // namespace dev
}  // namespace hlsp2p
