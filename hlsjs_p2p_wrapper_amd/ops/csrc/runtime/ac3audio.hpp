// AC-3 / E-AC-3 audio of one demuxed and remuxed segment (docs/AC3AUDIO.md holds the rules).  The
// sequential host implementation; kernels/ac3_audio.hip reproduces its output exactly, tables and
// bytes.
//
// The reference project has no Dolby path: whole syncframes become the samples of an 'ac-3' / 'ec-3'
// track (ETSI TS 102 366 Annex F), as whole MPEG audio frames do in runtime/mpegaudio.hpp.
#pragma once
#include <cstdint>

#include "grammar.hpp"

namespace hlsp2p {
namespace es {

// row layouts (Ac3info, Ac3Status): shared/layout.hpp; the scratch is mpa_scratch

// One segment behind remux_segment (and behind mpeg_audio_segment where that ran).
//   s:           as remux_segment took it (max_nal is not used)
//   region:      bytes of the segment's output region, the audio gap included
//   t.dframes:   int32[max_pes][kApesWords], -1 rows beyond the audio PES
//   t.ac3info:   int64[kAc3infoWords]
//   t.mpainfo:   int64[kMpainfoWords]: the row fragment_segment takes; for a segment that is not
//                Dolby audio a copy of t.mpa_in's kMpainfoWords, or kMpaNotMpegAudio without one
//   t.asamples:  the remux's int32[max_aframes][kAsampleWords]: the recorded frames' rows are written
//   t.rinfo:     the remux's row: Q, the frame total and the overflow bit are written
//   out:         the segment's output region; the audio box header and its payload are written
// A segment that is not Dolby audio, or has no counting frame at the start of audio PES 0, keeps
// every byte of asamples, rinfo and out.
void ac3_audio_segment(Segment s, int64_t region, int64_t max_aframes, const Ac3Tables& t, uint8_t* out);

}  // namespace es
}  // namespace hlsp2p
