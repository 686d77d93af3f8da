// The three device steps of a parameter-set kernel (codec_config.hip for H.264, hevc_config.hip
// for HEVC), each defined here once: the row search by wave ballot, the funnel copy of one NAL
// unit, and the ballot / popcount-prefix compaction of an RBSP.  One 256-thread workgroup per
// segment, wave64; every function is called by the whole workgroup unless it says otherwise.
#pragma once
#include "common.h"
#include "grammar.hpp"

namespace hlsp2p {
namespace dev {

constexpr int kPsThreads = 256;
constexpr int kPsWaves = kPsThreads / 64;
constexpr int kPsNone = 0x7fffffff;
static_assert(es::kMaxPsLimit / es::kPsAlign <= 64, "a wave copies a parameter set, a lane per 16 bytes");
static_assert(es::kPsAlign == 16 && es::kNalWords == 4, "16-byte stores, 16-byte NAL rows");

// a. The lowest row k < R of each of the N NAL types that has a length: rounds of 256 rows, one
// 16-byte load per lane, a wave ballot per type, the lowest row of each through s_found[N] (LDS,
// kPsNone in every slot and a barrier behind that before the call).  R is workgroup-uniform; the
// round loop ends once every type is found.  s_found is readable by every thread on return.
template <int N>
__device__ __forceinline__ void ps_find_rows(const v4i* __restrict__ rows, int R, const int (&types)[N],
                                             int* s_found) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int kb = 0; kb < R; kb += kPsThreads) {
    const int k = kb + tid;
    int type = -1;
    if (k < R) {
      const v4i row = rows[k];
      if (row[es::kNalLength] > 0) type = row[es::kNalType];
    }
    unsigned long long m[N];
#pragma unroll
    for (int w = 0; w < N; ++w) m[w] = __ballot(type == types[w]);
    if (lane == 0) {
#pragma unroll
      for (int w = 0; w < N; ++w)
        if (m[w]) atomicMin(&s_found[w], kb + wave * 64 + __builtin_ctzll(m[w]));
    }
    __syncthreads();
    bool done = true;
#pragma unroll
    for (int w = 0; w < N; ++w) done = done && s_found[w] != kPsNone;
    __syncthreads();  // every wave has read the round's result before the next round may change it
    if (done) break;
  }
}

// b. This lane's 16 bytes of one stored NAL unit: bytes [src + 16 lane, ..) of the segment's ES
// through its buffer resource (es_dev.h es_segment_rsrc: a load beyond the ES tensor yields
// zeros), at the NAL's alignment (load16_unaligned) and masked to the stored length
// min(len, max_ps).  Lanes behind the stored length get zeros.  For the lanes of one wave with
// 16 lane < max_ps.
__device__ __forceinline__ v4u ps_copy_lane(__amdgpu_buffer_rsrc_t rsrc, int src, int len, int max_ps, int lane) {
  const int stored = len < max_ps ? len : max_ps;
  const int left = stored - lane * 16;  // bytes of this lane's 16 that are stored
  v4u q = {0, 0, 0, 0};
  if (left > 0) {
    q = load16_unaligned(rsrc, src + lane * 16);
#pragma unroll
    for (int d = 0; d < 4; ++d) {  // zero behind the stored bytes
      const int keep = left - 4 * d;
      if (keep <= 0) q[d] = 0;
      else if (keep < 4) q[d] &= (1u << (8 * keep)) - 1u;
    }
  }
  return q;
}

// c. The RBSP of the stored NAL unit s_raw[0 .. n) behind its `header` bytes: a lane per byte
// flags emulation prevention from its two raw predecessors; a ballot and popcount prefix with a
// carry across waves (s_wave[kPsWaves], LDS) and rounds compacts the kept bytes into s_rbsp.
// n is workgroup-uniform; returns the RBSP's length.  A barrier stands behind the last store.
__device__ __forceinline__ int ps_unescape(const uint8_t* s_raw, int n, int header, uint8_t* s_rbsp, int* s_wave) {
  const int tid = threadIdx.x, lane = tid & 63;
  int carry = 0;
  for (int jb = 0; jb < n; jb += kPsThreads) {
    const int j = jb + tid;
    bool keep = false;
    uint8_t b = 0;
    if (j >= header && j < n) {
      b = s_raw[j];
      keep = j < 2 || !es::is_emulation_prevention(s_raw[j - 2], s_raw[j - 1], b);
    }
    const int inc = __popcll(__ballot(keep) & (~0ull >> (63 - lane)));  // kept bytes up to this lane's
    const WgPrefix<int> p = wg_exclusive_prefix<kPsWaves>(inc, keep ? 1 : 0, s_wave);
    if (keep) s_rbsp[carry + p.before] = b;
    carry += p.total;
    __syncthreads();  // s_wave is free again
  }
  return carry;
}

}  // namespace dev
}  // namespace hlsp2p
