// Sample index of one demuxed segment: NAL units and access units of the video ES, ADTS
// frames of the audio ES (docs/ESINDEX.md holds the rules).  The sequential host
// implementation; kernels/es_index.hip reproduces its output exactly.
//
// In the reference this happens inside hls.js's TS demuxer (Annex-B start-code scan and the
// ADTS header walk) before anything is buffered; here it is an index over the ES bytes the
// demux left in place: nothing is copied and emulation-prevention bytes stay.
#pragma once
#include <cstdint>

#include "grammar.hpp"

namespace hlsp2p {
namespace es {

// row layouts (NalRow, AuRow, ApesRow, Sinfo), status bits and access-unit flags: shared/layout.hpp

// Index one segment.
//   s.es:      the segment's [video ES | audio ES | id3 ES]; `s.cap` bytes are readable
//   s.info:    the demux info row (int64[ts::kInfoWords]); byte counts are clamped to `s.cap`
//   s.pes:     the demux PES table int64[ts::kClasses][max_pes][ts::kPesWords]
//   t.nal:     int32[max_nal][kNalWords], -1 rows beyond
//   t.au:      int32[max_pes][kAuWords], -1 rows beyond
//   t.aframes: int32[max_pes][kApesWords] per audio PES, -1 rows beyond
//   t.sinfo:   int64[kSinfoWords]
void index_segment(Segment s, const IndexTables<int32_t, int64_t>& t);

}  // namespace es
}  // namespace hlsp2p
