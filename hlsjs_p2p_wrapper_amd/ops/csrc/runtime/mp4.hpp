// Demux of one fragmented-MP4 (CMAF) media segment (docs/FMP4DEMUX.md holds the rules): the box
// tree is read for timing (tfdt, trun), the length-prefixed NAL units of the video samples are
// indexed in the layout of index_segment, and emsg boxes become rows.  No payload moves.  The
// sequential host implementation; kernels/mp4_demux.hip reproduces its output exactly.
#pragma once
#include <cstdint>

#include "grammar.hpp"

namespace hlsp2p {
namespace mp4 {

// row layouts (Minfo, RunRow, EmsgRow, ...), status bits and Tables / Limits: shared/layout.hpp

// segment b of a batch's tables
inline Tables tables_at(const Tables& t, const Limits& l, int64_t b) {
  return {t.minfo + b * kMinfoWords,
          t.msamples + table_words(b, kTracks * l.max_pes, kMsampleWords),
          t.runs + table_words(b, l.max_run, kRunWords),
          t.emsg + table_words(b, l.max_emsg, kEmsgWords),
          t.info + b * ts::kInfoWords,
          t.pes + ts::pes_words(b, l.max_pes),
          {t.ix.nal + table_words(b, l.max_nal, es::kNalWords), t.ix.au + table_words(b, l.max_pes, es::kAuWords),
           t.ix.aframes + table_words(b, l.max_pes, es::kApesWords), t.ix.sinfo + b * es::kSinfoWords}};
}

// One segment.
//   S, n:   the segment's bytes, only read; n < 2^31
//   tracks: kTracks rows of kTrackWords
//   lim:    max_pes, max_nal positive; max_moof, max_run, max_emsg max_rows_ok
void demux_segment(const uint8_t* S, int64_t n, const int64_t* tracks, const Limits& lim, const Tables& out);

}  // namespace mp4
}  // namespace hlsp2p
