// cenc (ISO/IEC 23001-7 AES-128-CTR, HLS SAMPLE-AES-CTR on fragmented MP4) decryption of one
// demuxed segment into a copy (docs/CENC.md holds the rules).  The sequential host
// implementation; kernels/cenc.hip reproduces its output exactly.
#pragma once
#include <cstdint>

#include "cbcs.hpp"

namespace hlsp2p {
namespace mp4 {

// row layouts (ProtRow, CnInfo, CnRangeRow), status bits (CbStatus): shared/layout.hpp

// One segment.
//   S, n:     the source bytes, only read; n < 2^31
//   prot:     kTracks rows of kProtWords; const_iv: kTracks x 16 bytes; iv: 16 bytes
//   erk:      44 words, aes::expand_key_enc
//   dst:      n bytes that hold a copy of S; the bytes of the recorded ranges are decrypted there
//   ranges:   max_range rows of kCnRangeWords; cinfo: kCnInfoWords
void cenc_segment(const uint8_t* S, int64_t n, const CbcsDemux& md, const int64_t* prot, const uint8_t* const_iv,
                  const uint8_t* iv, const uint32_t* erk, int64_t max_range, uint8_t* dst, int32_t* ranges,
                  int64_t* cinfo);

}  // namespace mp4
}  // namespace hlsp2p
