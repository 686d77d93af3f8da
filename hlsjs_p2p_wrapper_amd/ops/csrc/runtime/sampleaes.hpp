// HLS SAMPLE-AES decryption of one demuxed and indexed segment in place (docs/SAMPLEAES.md holds
// the rules): protected H.264 slice NALs are unescaped and every tenth 16-byte block of them is
// decrypted, and so are the whole blocks of every counted ADTS frame behind its 16-byte leader.
// The sequential host implementation; kernels/sample_aes.hip reproduces its output exactly.
#pragma once
#include <cstdint>

#include "grammar.hpp"

namespace hlsp2p {
namespace es {

// row layout (Sainfo), status bits (SaStatus) and the block geometry: shared/layout.hpp

// One segment.
//   s:      as index_segment took it, with es writable
//   es:     s.es, the bytes that are rewritten
//   ix:     what index_segment wrote (rows are used as found, clamped); nal[..][kNalLength] of a
//           protected row becomes its unescaped length
//   drk:    aes::expand_key_dec of the segment's key
//   iv:     16 bytes
//   sainfo: int64[kSaWords]
void sample_decrypt_segment(Segment s, uint8_t* es, const IndexTables<int32_t, const int64_t>& ix,
                            const uint32_t drk[kAesRoundKeyWords], const uint8_t iv[kAesBlock], int64_t* sainfo);

}  // namespace es
}  // namespace hlsp2p
