// Codec configuration of one demuxed and indexed segment for the fMP4 init segment
// (docs/INITSEGMENT.md holds the rules): the first SPS and PPS NAL units, what the SPS says, and
// the three ADTS header fields of an AudioSpecificConfig.  The sequential host implementation;
// kernels/codec_config.hip reproduces its output exactly.
//
// In the reference this is the part of hls.js's TS demuxer that reads the SPS (exp-golomb.js) and
// the ADTS header (adts.js) into the track config the MP4 remuxer builds its init segment from.
// The boxes themselves are host work (player/fmp4.py).
#pragma once
#include <cstdint>

#include "grammar.hpp"

namespace hlsp2p {
namespace es {

// row layout (Cinfo), status bits (ConfigStatus) and the limits of max_ps: shared/layout.hpp

struct SpsRow {
  int32_t rbsp_bytes;
  bool ok;
  SpsFields f;
};
// One stored SPS NAL unit b[0 .. n) (header byte first, emulation prevention kept): unescape, then sps_parse.
SpsRow parse_sps_nal(const uint8_t* b, int64_t n);

// The configuration of one segment.
//   s:      as index_segment took it
//   ix:     what index_segment wrote (rows are used as found, clamped)
//   max_ps: max_ps_ok(max_ps)
//   ps:     uint8[kPsRows][max_ps], zero behind the stored bytes
//   cinfo:  int32[kCinfoWords]
void config_segment(Segment s, const IndexTables<const int32_t, const int64_t>& ix, int64_t max_ps, uint8_t* ps,
                    int32_t* cinfo);

}  // namespace es
}  // namespace hlsp2p
