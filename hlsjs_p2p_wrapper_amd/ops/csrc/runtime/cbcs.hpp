// cbcs (ISO/IEC 23001-7, HLS SAMPLE-AES on fragmented MP4) decryption of one demuxed segment into
// a copy (docs/CBCS.md holds the rules).  The sequential host implementation;
// kernels/cbcs.hip reproduces its output exactly.
#pragma once
#include <cstdint>

#include "grammar.hpp"

namespace hlsp2p {
namespace mp4 {

// row layouts (ProtRow, CbInfo, RangeRow), status bits: shared/layout.hpp

// One segment's rows of demux_segment's tables, only read.
struct CbcsDemux {
  const int64_t *minfo, *runs, *info, *pes;  // pes: [ts::kClasses][max_pes][ts::kPesWords]
  const int32_t* msamples;                   // [kTracks][max_pes][kMsampleWords]
  int64_t max_pes, max_run;
};

// One segment.
//   S, n:     the source bytes, only read; n < 2^31
//   prot:     kTracks rows of kProtWords; const_iv: kTracks x 16 bytes; iv: 16 bytes
//   drk:      44 words, aes::expand_key_dec
//   dst:      n bytes that hold a copy of S; the cipher blocks of the recorded ranges are decrypted there
//   ranges:   max_range rows of kRangeWords; cinfo: kCbInfoWords
void cbcs_segment(const uint8_t* S, int64_t n, const CbcsDemux& md, const int64_t* prot, const uint8_t* const_iv,
                  const uint8_t* iv, const uint32_t* drk, int64_t max_range, uint8_t* dst, int32_t* ranges,
                  int64_t* cinfo);

}  // namespace mp4
}  // namespace hlsp2p
