// Sample index of one demuxed segment: NAL units and access units of the video ES, ADTS
// frames of the audio ES (docs/ESINDEX.md holds the rules).  The sequential host
// implementation; kernels/es_index.hip reproduces its output exactly.
//
// In the reference this happens inside hls.js's TS demuxer (Annex-B start-code scan and the
// ADTS header walk) before anything is buffered; here it is an index over the ES bytes the
// demux left in place: nothing is copied and emulation-prevention bytes stay.
#pragma once
#include <cstdint>

#include "layout.hpp"

namespace hlsp2p {
namespace es {

// sinfo[] row layout, status bits and access-unit flags: shared/layout.hpp

// Index one segment.
//   es:      the segment's [video ES | audio ES | id3 ES]; `cap` bytes are readable
//   info:    the demux info row (int64[ts::kInfoWords]); byte counts are clamped to `cap`
//   pes:     the demux PES table int64[ts::kClasses][max_pes][3]
//   nal:     int32[max_nal][4] = (offset, length, type, access unit), -1 rows beyond
//   au:      int32[max_pes][4] = (first NAL, NAL count, flags, size), -1 rows beyond
//   aframes: int32[max_pes][2] = (ADTS frames, bytes consumed) per audio PES, -1 rows beyond
//   sinfo:   int64[kSinfoWords]
void index_segment(const uint8_t* es, int64_t cap, const int64_t* info, const int64_t* pes, int64_t max_pes,
                   int64_t max_nal, int32_t* nal, int32_t* au, int32_t* aframes, int64_t* sinfo);

}  // namespace es
}  // namespace hlsp2p
