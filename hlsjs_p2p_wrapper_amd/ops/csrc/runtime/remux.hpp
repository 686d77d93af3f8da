// Remux of one demuxed and indexed segment to fMP4 samples and mdat boxes (docs/REMUX.md holds
// the rules).  The sequential host implementation; kernels/remux.hip reproduces its output
// exactly, tables and bytes.
//
// In the reference this is hls.js's MP4 remuxer between the TS demuxer and the SourceBuffer:
// Annex-B start codes become 4-byte lengths, ADTS headers fall away, and per-sample rows carry
// what a trun box needs.  The moof itself is host work (player/fmp4.py).
#pragma once
#include <cstdint>

#include "layout.hpp"

namespace hlsp2p {
namespace es {

// rinfo[] row layout and status bits, region and scratch sizes: shared/layout.hpp

// Remux one segment.
//   es / cap / info / pes:      as index_segment took them
//   nal / au / aframes / sinfo: what index_segment wrote (rows are used as found, clamped)
//   vsamples: int32[max_pes][5] = (offset, size, duration, cts, flags), -1 rows beyond
//   asamples: int32[max_aframes][2] = (offset, size), -1 rows beyond
//   rinfo:    int64[kRinfoWords]
//   out:      the segment's output region, remux_out_bytes(cap, max_nal) bytes writable; only
//             the two box headers and the two payloads are written
void remux_segment(const uint8_t* es, int64_t cap, const int64_t* info, const int64_t* pes, int64_t max_pes,
                   int64_t max_nal, const int32_t* nal, const int32_t* au, const int32_t* aframes,
                   const int64_t* sinfo, int64_t max_aframes, int32_t* vsamples, int32_t* asamples, int64_t* rinfo,
                   uint8_t* out);

}  // namespace es
}  // namespace hlsp2p
