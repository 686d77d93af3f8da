// Demux of one packed-audio segment (docs/PACKEDAUDIO.md holds the rules): leading ID3v2 tags, the
// transport stream timestamp of their PRIV frame, and raw ADTS frames back to back, four to an
// audio PES row.  No payload moves.  The sequential host implementation;
// kernels/packed_audio.hip reproduces its output exactly.
#pragma once
#include <algorithm>
#include <cstdint>

#include "grammar.hpp"

namespace hlsp2p {
namespace es {

// row layouts (Painfo, PackedStatus) and PackedTables: shared/layout.hpp

// segment b of a batch's tables
inline PackedTables packed_tables_at(const PackedTables& t, int64_t max_pes, int64_t b) {
  return {t.info + b * ts::kInfoWords,
          t.pes + ts::pes_words(b, max_pes),
          {t.ix.nal + table_words(b, kPackedNalRows, kNalWords), t.ix.au + table_words(b, max_pes, kAuWords),
           t.ix.aframes + table_words(b, max_pes, kApesWords), t.ix.sinfo + b * kSinfoWords},
          t.painfo + b * kPainfoWords};
}

// One segment: S, n its bytes, only read, n < 2^31; max_pes positive.
void packed_segment(const uint8_t* S, int64_t n, int64_t max_pes, const PackedTables& out);

// The passes of packed_segment over a reader of the caller: rd answers the tag rules (u8, be32 of
// the segment), S the frame walk; n >= 0.
template <class R>
void packed_segment_with(R rd, const uint8_t* S, int64_t n, int64_t max_pes, const PackedTables& out) {
  std::fill(out.pes, out.pes + ts::pes_words(1, max_pes), int64_t(-1));
  std::fill(out.ix.nal, out.ix.nal + table_words(1, kPackedNalRows, kNalWords), -1);
  std::fill(out.ix.au, out.ix.au + table_words(1, max_pes, kAuWords), -1);
  std::fill(out.ix.aframes, out.ix.aframes + table_words(1, max_pes, kApesWords), -1);
  const PackedTags tags = packed_tags(rd, n);

  // ---- the frame chain; a group's row is written as its frames are met
  int64_t n_frames = 0, q = tags.T, rate = 0, chans = 0;
  int64_t* audio = out.pes + table_words(1, max_pes, ts::kPesWords);
  int32_t* af = out.ix.aframes;
  int64_t group_start = q;
  if (!(tags.status & kPaBadId3)) {
    for (;;) {
      const AdtsFrame f = adts_frame_at(S, q, n);
      if (f.len == 0) break;
      if (n_frames == 0) {
        rate = adts_rate((S[q + 2] >> 2) & 15);
        chans = adts_channels(S[q + 2], S[q + 3]);
      }
      const int64_t k = n_frames / kPackedFramesPerPes;
      if (n_frames % kPackedFramesPerPes == 0) {
        group_start = q;
        if (k < max_pes) {
          audio[ts::kPesWords * k + ts::kPesEsOffset] = q - tags.T;
          af[kApesWords * k + kApesFrames] = 0;
        }
      }
      q += f.len;
      ++n_frames;
      if (k < max_pes) {
        af[kApesWords * k + kApesFrames] += 1;
        af[kApesWords * k + kApesUsed] = static_cast<int32_t>(q - group_start);
      }
    }
  }
  const PackedSummary s = packed_summary(tags, n_frames, q, rate, chans, n, max_pes);
  const int64_t rec = std::min(packed_groups(n_frames), max_pes);
  for (int64_t k = 0; k < rec; ++k) {
    const int64_t stamp = packed_stamp(s.ts, k, s.rate);
    audio[ts::kPesWords * k + ts::kPesPts] = stamp;
    audio[ts::kPesWords * k + ts::kPesDts] = stamp;
  }
  if (s.T > 0) {
    int64_t* id3 = out.pes + table_words(2, max_pes, ts::kPesWords);
    id3[ts::kPesEsOffset] = 0;
    id3[ts::kPesPts] = s.ts;
    id3[ts::kPesDts] = s.ts;
  }
  for (int i = 0; i < ts::kInfoWords; ++i) out.info[i] = packed_info_word(i, s, max_pes);
  for (int i = 0; i < kSinfoWords; ++i) out.ix.sinfo[i] = packed_sinfo_word(i, s);
  for (int i = 0; i < kPainfoWords; ++i) out.painfo[i] = packed_painfo_word(i, s);
}

}  // namespace es
}  // namespace hlsp2p
