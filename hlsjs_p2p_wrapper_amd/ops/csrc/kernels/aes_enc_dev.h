// AES-128 forward rounds on the bulk decrypt's 160 KiB conflict-free LDS image (aes_dev.h), for
// the AES-CTR keystream of cenc.hip.
//
// The image is filled by aes_image_fill with TeL (Te0 in little-endian column form,
// 2s | s << 8 | s << 16 | 3s << 24) in place of TdL and the S-box in place of InvSbox: Te1..Te3 are
// byte rotations of Te0 exactly as Td1..Td3 are of Td0, so the fill's rotations give them, and
// the addressing (aes_image_bases, AES_TDA, AES_IS) is unchanged.  What differs is which state
// word feeds which table: ShiftRows moves row k of column c from column c + k, where
// InvShiftRows takes it from column c - k.  AES_ROUND_XORS is shared.
//
// Round keys: per segment the 44 forward round-key words, little-endian (host pre-swapped):
// [0..3] whitening, [4r..4r+3] round r (1..9), [40..43] last round.
#pragma once
#include "aes_dev.h"

namespace hlsp2p {
namespace dev {

#define AES_ENC_ROUND_READS(v, s)                                                                                 \
  do {                                                                                                            \
    uint32_t a_[16];                                                                                              \
    a_[0] = AES_TDA(0, s[0], 0); a_[1] = AES_TDA(1, s[1], 1); a_[2] = AES_TDA(2, s[2], 2); a_[3] = AES_TDA(3, s[3], 3);     \
    a_[4] = AES_TDA(0, s[1], 0); a_[5] = AES_TDA(1, s[2], 1); a_[6] = AES_TDA(2, s[3], 2); a_[7] = AES_TDA(3, s[0], 3);     \
    a_[8] = AES_TDA(0, s[2], 0); a_[9] = AES_TDA(1, s[3], 1); a_[10] = AES_TDA(2, s[0], 2); a_[11] = AES_TDA(3, s[1], 3);   \
    a_[12] = AES_TDA(0, s[3], 0); a_[13] = AES_TDA(1, s[0], 1); a_[14] = AES_TDA(2, s[1], 2); a_[15] = AES_TDA(3, s[2], 3); \
    _Pragma("unroll") for (int q_ = 0; q_ < 16; ++q_) v[q_] = AES_LDS32(a_[q_]);                                  \
  } while (0)

// final round: o = ShiftRows/SubBytes(s) ^ k through the byte-replicated S-box image; the two
// v_perm of AES_FINAL pick the four output bytes into disjoint byte lanes
#define AES_ENC_FINAL(s0, s1, s2, s3, o0, o1, o2, o3, k)                                                        \
  o0 = __builtin_amdgcn_bitop3_b32(__builtin_amdgcn_perm(AES_IS(s1, 1), AES_IS(s0, 0), 0x0c0c0500u),               \
                                   __builtin_amdgcn_perm(AES_IS(s3, 3), AES_IS(s2, 2), 0x07020c0cu), (k)[0], 0x96);  \
  o1 = __builtin_amdgcn_bitop3_b32(__builtin_amdgcn_perm(AES_IS(s2, 1), AES_IS(s1, 0), 0x0c0c0500u),               \
                                   __builtin_amdgcn_perm(AES_IS(s0, 3), AES_IS(s3, 2), 0x07020c0cu), (k)[1], 0x96);  \
  o2 = __builtin_amdgcn_bitop3_b32(__builtin_amdgcn_perm(AES_IS(s3, 1), AES_IS(s2, 0), 0x0c0c0500u),               \
                                   __builtin_amdgcn_perm(AES_IS(s1, 3), AES_IS(s0, 2), 0x07020c0cu), (k)[2], 0x96);  \
  o3 = __builtin_amdgcn_bitop3_b32(__builtin_amdgcn_perm(AES_IS(s0, 1), AES_IS(s3, 0), 0x0c0c0500u),               \
                                   __builtin_amdgcn_perm(AES_IS(s2, 3), AES_IS(s1, 2), 0x07020c0cu), (k)[3], 0x96);

// Rounds 1..9 of N independent blocks, software-pipelined in source order as
// AES_ROUNDS_PIPELINED does: block j's 16 LDS reads are issued before block j-1's XORs.
#define AES_ENC_ROUNDS_PIPELINED(N, st, rk)                                                                       \
  _Pragma("unroll") for (int r_ = 1; r_ < 10; ++r_) {                                                             \
    const uint32_t* k_ = (rk) + 4 * r_;                                                                           \
    uint32_t v_[2][16];                                                                                           \
    AES_ENC_ROUND_READS(v_[0], st[0]);                                                                            \
    _Pragma("unroll") for (int j_ = 1; j_ < (N); ++j_) {                                                          \
      AES_ENC_ROUND_READS(v_[j_ & 1], st[j_]);                                                                    \
      AES_ROUND_XORS(st[j_ - 1], v_[(j_ - 1) & 1], k_);                                                           \
    }                                                                                                             \
    AES_ROUND_XORS(st[(N) - 1], v_[((N) - 1) & 1], k_);                                                           \
  }

}  // namespace dev
}  // namespace hlsp2p
