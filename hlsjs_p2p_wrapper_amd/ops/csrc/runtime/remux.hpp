// Remux of one demuxed and indexed segment to fMP4 samples and mdat boxes (docs/REMUX.md holds
// the rules).  The sequential host implementation; kernels/remux.hip reproduces its output
// exactly, tables and bytes.
//
// In the reference this is hls.js's MP4 remuxer between the TS demuxer and the SourceBuffer:
// Annex-B start codes become 4-byte lengths, ADTS headers fall away, and per-sample rows carry
// what a trun box needs.  The moof itself is host work (player/fmp4.py).
#pragma once
#include <cstdint>

#include "grammar.hpp"

namespace hlsp2p {
namespace es {

// row layouts (VsampleRow, AsampleRow, Rinfo) and status bits, region and scratch sizes: shared/layout.hpp

// Remux one segment.
//   s:          as index_segment took it
//   ix:         what index_segment wrote (rows are used as found, clamped)
//   t.vsamples: int32[max_pes][kVsampleWords], -1 rows beyond
//   t.asamples: int32[max_aframes][kAsampleWords], -1 rows beyond
//   t.rinfo:    int64[kRinfoWords]
//   out:        the segment's output region, remux_out_bytes(cap, max_nal) + audio_gap bytes
//               writable; only the two box headers and the two payloads are written
//   audio_gap:  free bytes in front of the audio box (a non-negative multiple of 16): room for
//               the audio moof of runtime/fragment.cpp
void remux_segment(Segment s, const IndexTables<const int32_t, const int64_t>& ix, int64_t max_aframes,
                   const RemuxTables& t, uint8_t* out, int64_t audio_gap = 0);

}  // namespace es
}  // namespace hlsp2p
