// The moof boxes of one remuxed segment (docs/FRAGMENT.md holds the rules).  The sequential host
// implementation; kernels/fragment.hip reproduces its output exactly, finfo row and bytes.
//
// In the reference this is the moof half of hls.js's MP4 remuxer (mp4-generator.js moof / traf /
// trun) with the timestamp handling in front of it (_initPTS, _PTSNormalize): the remux has left
// both mdat boxes and the sample tables, this step writes each track's moof directly in front of
// its mdat, so a fragment is one byte range.
#pragma once
#include <cstdint>

#include "grammar.hpp"

namespace hlsp2p {
namespace es {

// row layouts (Finfo, Fparam), status bits and the sizes of the boxes: shared/layout.hpp

// Write one segment's two moof boxes.
//   rinfo, vsamples, asamples: what remux_segment wrote (rows are used as found, clamped)
//   rate:      the index's audio sample rate (sinfo[kAudioSampleRate])
//   fparam:    the segment's fparams row; kFpOutOff is not used here
//   audio_gap: what remux_segment took, >= frag_audio_gap(max_aframes); the region holds at
//              least audio_gap + 32 bytes
//   out:       where the segment's video mdat starts: frag_headroom(max_pes) bytes in front of
//              it and fparam[kFpRegion] bytes from it on are writable.  Only the two moof boxes
//              are written: the video one ends at out, the audio one at out + A0.
//   finfo:     int64[kFinfoWords]
//   mpainfo:   the segment's row of mpeg_audio_segment, or null: with a config its rate and frame
//              replace `rate` and the AAC frame (docs/MPEGAUDIO.md)
void fragment_segment(const int64_t* rinfo, const int32_t* vsamples, const int32_t* asamples, int64_t rate,
                      const int64_t* fparam, int64_t max_pes, int64_t max_aframes, int64_t audio_gap, uint8_t* out,
                      int64_t* finfo, const int64_t* mpainfo = nullptr);

}  // namespace es
}  // namespace hlsp2p
