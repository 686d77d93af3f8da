// MPEG audio (MPEG-1/2/2.5 Layer I-III) of one demuxed and remuxed segment (docs/MPEGAUDIO.md holds
// the rules).  The sequential host implementation; kernels/mpeg_audio.hip reproduces its output
// exactly, tables and bytes.
//
// In the reference this is hls.js's tsdemuxer _parseMPEGPES with demux/mpegaudio.js: whole frames,
// header included, become the samples of an mp4a track with object type 0x6B / 0x69.
#pragma once
#include <cstdint>

#include "grammar.hpp"

namespace hlsp2p {
namespace es {

// row layouts (Mpainfo, MpaStatus) and the scratch size: shared/layout.hpp

// One segment behind remux_segment.
//   s:           as remux_segment took it (max_nal is not used)
//   region:      bytes of the segment's output region, the audio gap included
//   t.mframes:   int32[max_pes][kApesWords], -1 rows beyond the audio PES
//   t.mpainfo:   int64[kMpainfoWords]
//   t.asamples:  the remux's int32[max_aframes][kAsampleWords]: the recorded frames' rows are written
//   t.rinfo:     the remux's row: Q, the frame total and the overflow bit are written
//   out:         the segment's output region; the audio box header and its payload are written
// A segment that is not MPEG audio, or has no counting frame at the start of audio PES 0, keeps
// every byte of asamples, rinfo and out.
void mpeg_audio_segment(Segment s, int64_t region, int64_t max_aframes, const MpaTables& t, uint8_t* out);

}  // namespace es
}  // namespace hlsp2p
