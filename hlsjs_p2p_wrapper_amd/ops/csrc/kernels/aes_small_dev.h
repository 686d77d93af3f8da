// A small AES-128 block decrypt for kernels whose ciphertext is a minor share of their bytes
// (sample_aes.hip): one 1 KiB Td table (TdL, little-endian column form, the other three are
// rotations of it by v_alignbit), the 256-byte inverse S-box and one segment's 44 round keys in
// LDS, 1.4 KiB per workgroup.  Same tables (ops.aes.device_tables) and the same round-key layout
// (round_keys_le) as the bulk decrypt; aes_dev.h and aes_cbc.hip are not involved.  Lookups of
// different lanes may hit one bank: accepted, see docs/SAMPLEAES.md.
//
// Round keys: 44 little-endian words of the equivalent inverse cipher: [0..3] initial whitening,
// [4r..4r+3] round r (1..9), [40..43] last round.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace hlsp2p {
namespace dev {

struct AesSmallLds {
  uint32_t td[256];
  uint32_t rk[44];
  uint8_t isb[256];
};

// Fill by a workgroup of at least 256 threads; the caller synchronises.
__device__ __forceinline__ void aes_small_fill(AesSmallLds& s, const uint32_t* __restrict__ tdl_g,
                                               const uint8_t* __restrict__ isb_g, const uint32_t* __restrict__ rk_g,
                                               int tid) {
  if (tid < 256) {
    s.td[tid] = tdl_g[tid];
    s.isb[tid] = isb_g[tid];
  }
  if (tid < 44) s.rk[tid] = rk_g[tid];
}

__device__ __forceinline__ uint32_t aes_small_rotl(uint32_t v, int bits) {
  return __builtin_amdgcn_alignbit(v, v, 32 - bits);
}

// One column of a middle round: the four bytes come from the columns c, c+3, c+2, c+1 (InvShiftRows).
__device__ __forceinline__ uint32_t aes_small_col(const AesSmallLds& s, uint32_t a, uint32_t b, uint32_t c, uint32_t d,
                                                  uint32_t k) {
  return s.td[a & 0xff] ^ aes_small_rotl(s.td[(b >> 8) & 0xff], 8) ^ aes_small_rotl(s.td[(c >> 16) & 0xff], 16) ^
         aes_small_rotl(s.td[d >> 24], 24) ^ k;
}
__device__ __forceinline__ uint32_t aes_small_last(const AesSmallLds& s, uint32_t a, uint32_t b, uint32_t c, uint32_t d,
                                                   uint32_t k) {
  return (static_cast<uint32_t>(s.isb[a & 0xff]) | (static_cast<uint32_t>(s.isb[(b >> 8) & 0xff]) << 8) |
          (static_cast<uint32_t>(s.isb[(c >> 16) & 0xff]) << 16) | (static_cast<uint32_t>(s.isb[d >> 24]) << 24)) ^ k;
}

// D_key(c): c and the result are the block's four dwords as loaded (little-endian).
__device__ __forceinline__ uint4 aes_small_decrypt(const AesSmallLds& s, uint4 c) {
  uint32_t s0 = c.x ^ s.rk[0], s1 = c.y ^ s.rk[1], s2 = c.z ^ s.rk[2], s3 = c.w ^ s.rk[3];
#pragma unroll 1
  for (int r = 1; r < 10; ++r) {
    const uint32_t* k = s.rk + 4 * r;
    const uint32_t t0 = aes_small_col(s, s0, s3, s2, s1, k[0]);
    const uint32_t t1 = aes_small_col(s, s1, s0, s3, s2, k[1]);
    const uint32_t t2 = aes_small_col(s, s2, s1, s0, s3, k[2]);
    const uint32_t t3 = aes_small_col(s, s3, s2, s1, s0, k[3]);
    s0 = t0; s1 = t1; s2 = t2; s3 = t3;
  }
  const uint32_t* k = s.rk + 40;
  return uint4{aes_small_last(s, s0, s3, s2, s1, k[0]), aes_small_last(s, s1, s0, s3, s2, k[1]),
               aes_small_last(s, s2, s1, s0, s3, k[2]), aes_small_last(s, s3, s2, s1, s0, k[3])};
}

}  // namespace dev
}  // namespace hlsp2p
