// Device helpers of the kernels that read fragmented-MP4 segments where they lie (mp4_demux.hip,
// cbcs.hip, cenc.hip): the segment reader over a buffer resource, the 64-bit wave scan, the LDS
// search and the 16-byte store at any alignment.
#pragma once
#include "common.h"
#include "grammar.hpp"

namespace hlsp2p {
namespace dev {

typedef long long v2l __attribute__((ext_vector_type(2)));

// The segment's bytes through a buffer resource of n bytes rounded up to a dword and never beyond
// the tensor.  u8 keeps the 16 bytes from the last position asked for, so a box header, a trun
// entry or a NAL's length and header byte cost one load.
struct SegReader {
  __amdgpu_buffer_rsrc_t rsrc;
  int64_t at;
  v4u w;
  __device__ __forceinline__ int u8(int64_t p) {
    if (p < at || p >= at + 16) {
      at = p;
      w = load16_unaligned(rsrc, static_cast<int>(p));
    }
    const int k = static_cast<int>(p - at);
    return static_cast<int>((w[k >> 2] >> (8 * (k & 3))) & 0xff);
  }
  // four bytes at once: the two dwords around them, one v_alignbyte, one v_perm (bswap)
  __device__ __forceinline__ uint32_t be32(int64_t p) {
    if (p < at || p + 4 > at + 16) {
      at = p;
      w = load16_unaligned(rsrc, static_cast<int>(p));
    }
    const int k = static_cast<int>(p - at), i = k >> 2;  // k <= 12; an unaligned k has i <= 2
    const uint32_t lo = w[i], hi = i < 3 ? w[i + 1] : 0u;
    return __builtin_bswap32(__builtin_amdgcn_alignbyte(hi, lo, static_cast<uint32_t>(k & 3)));
  }
};
// the n bytes at buf + off of a tensor of buf_numel bytes; off, n and buf are wave-uniform
__device__ __forceinline__ SegReader mp4_reader(const uint8_t* buf, int64_t buf_numel, int64_t off, int n) {
  int64_t range = (static_cast<int64_t>(n) + 3) & ~int64_t(3);
  if (range > buf_numel - off) range = buf_numel - off;
  if (range < 0) range = 0;
  const uint64_t base = reinterpret_cast<uint64_t>(buf + off);
  const uint32_t lo = __builtin_amdgcn_readfirstlane(static_cast<uint32_t>(base));
  const uint32_t hi = __builtin_amdgcn_readfirstlane(static_cast<uint32_t>(base >> 32));
  const int bytes = __builtin_amdgcn_readfirstlane(static_cast<int>(range));
  SegReader rd;
  rd.rsrc = __builtin_amdgcn_make_buffer_rsrc(reinterpret_cast<uint8_t*>((static_cast<uint64_t>(hi) << 32) | lo), 0,
                                              bytes, 0x00020000);
  rd.at = -64;
  rd.w = v4u{0, 0, 0, 0};
  return rd;
}

// inclusive prefix sum of a 64-bit value over the wave64
__device__ __forceinline__ long long wave_scan64(long long v) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const long long t = __shfl_up(v, d);
    if (lane >= d) v += t;
  }
  return v;
}

// largest k in [0, K) with first[k] <= i; first ascends and first[0] <= i
__device__ __forceinline__ int last_le_lds(const long long* first, int K, long long i) {
  int lo = 0, hi = K;  // the answer is in [lo, hi)
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (first[mid] <= i) lo = mid;
    else hi = mid;
  }
  return lo;
}

// 16 bytes with the widest stores the address allows
__device__ __forceinline__ void cbcs_store16(uint8_t* p, const uint4& v) {
  const uint32_t w[4] = {v.x, v.y, v.z, v.w};
  const uintptr_t al = reinterpret_cast<uintptr_t>(p);
  if (!(al & 15)) {
    *reinterpret_cast<uint4*>(p) = v;
  } else if (!(al & 7)) {
    reinterpret_cast<uint2*>(p)[0] = uint2{v.x, v.y};
    reinterpret_cast<uint2*>(p)[1] = uint2{v.z, v.w};
  } else if (!(al & 3)) {
#pragma unroll
    for (int d = 0; d < 4; ++d) reinterpret_cast<uint32_t*>(p)[d] = w[d];
  } else if (!(al & 1)) {
#pragma unroll
    for (int d = 0; d < 8; ++d) reinterpret_cast<uint16_t*>(p)[d] = static_cast<uint16_t>(w[d >> 1] >> (16 * (d & 1)));
  } else {
#pragma unroll
    for (int d = 0; d < 16; ++d) p[d] = static_cast<uint8_t>(w[d >> 2] >> (8 * (d & 3)));
  }
}

}  // namespace dev
}  // namespace hlsp2p
