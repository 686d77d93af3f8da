// HEVC configuration of one demuxed and indexed segment for the hvc1 init segment
// (docs/INITSEGMENT.md holds the rules): the first VPS, SPS and PPS NAL units and what the SPS says
// up to its bit depths.  The sequential host implementation; kernels/hevc_config.hip reproduces
// its output exactly.  Audio stays in config_segment's cinfo row.  The boxes themselves are host
// work (player/fmp4.py).
#pragma once
#include <cstdint>

#include "grammar.hpp"

namespace hlsp2p {
namespace es {

// row layout (Hinfo), status bits (HevcStatus) and the limits of max_ps: shared/layout.hpp

struct HevcSpsRow {
  int32_t rbsp_bytes;
  bool ok;
  HevcSpsFields f;
};
// One stored SPS NAL unit b[0 .. n) (two header bytes first, emulation prevention kept): unescape, then hevc_sps_parse.
HevcSpsRow parse_hevc_sps_nal(const uint8_t* b, int64_t n);

// The HEVC configuration of one segment.
//   s:      as index_segment took it
//   ix:     what index_segment wrote (rows are used as found, clamped)
//   max_ps: max_ps_ok(max_ps)
//   hps:    uint8[kHpsRows][max_ps], zero behind the stored bytes
//   hinfo:  int32[kHinfoWords]
void hevc_config_segment(Segment s, const IndexTables<const int32_t, const int64_t>& ix, int64_t max_ps, uint8_t* hps,
                         int32_t* hinfo);

}  // namespace es
}  // namespace hlsp2p
