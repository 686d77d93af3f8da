// Host sample index: the serial loops that fill the rows.  The segment view and the codec,
// NAL-type and ADTS byte rules are shared/grammar.hpp (namespace es), the same functions
// kernels/es_index.hip calls.
#include "es.hpp"

#include <algorithm>
#include <vector>

namespace hlsp2p {
namespace es {

void index_segment(Segment s, const IndexTables<int32_t, int64_t>& t) {
  const int64_t max_pes = s.max_pes, max_nal = s.max_nal;
  int32_t *nal = t.nal, *au = t.au, *aframes = t.aframes;
  int64_t* sinfo = t.sinfo;
  std::fill(nal, nal + table_words(1, max_nal, kNalWords), -1);
  std::fill(au, au + table_words(1, max_pes, kAuWords), -1);
  std::fill(aframes, aframes + table_words(1, max_pes, kApesWords), -1);
  std::fill(sinfo, sinfo + kSinfoWords, int64_t(0));
  sinfo[kFirstKeyframeAu] = -1;
  s.cap = std::max<int64_t>(s.cap, 0);  // the host takes any cap: a negative one reads nothing
  const VideoSpan video = video_span(s);
  const bool hevc = video.hevc;
  int64_t status = video.supported ? 0 : kUnsupportedVideo;
  const uint8_t* V = s.es;
  const int64_t n = video.len;

  // ---- start codes, in offset order; one position past the table ends its last NAL
  std::vector<int64_t> p;  // start-code positions of the first max_nal + 1 NALs
  int64_t n_nal = 0;
  for (int64_t i = 0; i + 3 < n;) {
    if (V[i] == 0 && V[i + 1] == 0 && V[i + 2] == 1) {
      if (n_nal <= max_nal) p.push_back(i);
      ++n_nal;
      i += 3;
    } else {
      ++i;
    }
  }
  if (n_nal > max_nal) status |= kNalOverflow;
  const int64_t nn = std::min(n_nal, max_nal);

  // ---- NAL rows
  const int64_t m = video_rows(video, s.info[ts::kNumVideoPes], max_pes);  // the demux's count: one unit per PES
  const PesRows rows = pes_rows(s);
  const int64_t* vp = rows.video;
  int64_t a = -1;  // access unit of the current NAL: PES offsets ascend with the NAL starts
  for (int64_t k = 0; k < nn; ++k) {
    const int64_t b = p[k] + 3;
    int64_t e = n;
    if (k + 1 < n_nal) {
      const int64_t p1 = p[k + 1];
      const int64_t z1 = (p1 > 0 && V[p1 - 1] == 0) ? 1 : 0;
      e = std::max(b, p1 - z1);
    }
    while (a + 1 < m && pes_at(vp, a + 1, ts::kPesEsOffset) <= b) ++a;
    int32_t* row = nal + kNalWords * k;
    row[kNalOffset] = static_cast<int32_t>(b);
    row[kNalLength] = static_cast<int32_t>(e - b);
    row[kNalType] = e == b ? -1 : nal_type(hevc, V[b]);
    row[kNalAu] = static_cast<int32_t>(a);
  }

  // ---- access unit rows
  int64_t n_key = 0, first_key = -1;
  for (int64_t u = 0; u < m; ++u) {
    const int64_t next = u + 1 < m ? pes_at(vp, u + 1, ts::kPesEsOffset) : n;
    int32_t* row = au + kAuWords * u;
    row[kAuFirstNal] = -1;
    row[kAuNalCount] = 0;
    row[kAuFlags] = 0;
    row[kAuSize] = static_cast<int32_t>(next - pes_at(vp, u, ts::kPesEsOffset));
  }
  for (int64_t k = 0; k < nn; ++k) {
    const int64_t u = nal[kNalWords * k + kNalAu];
    if (u < 0) continue;
    int32_t* row = au + kAuWords * u;
    if (row[kAuNalCount] == 0) row[kAuFirstNal] = static_cast<int32_t>(k);
    ++row[kAuNalCount];
    row[kAuFlags] |= nal_flags(hevc, nal[kNalWords * k + kNalType]);
  }
  for (int64_t u = 0; u < m; ++u) {
    if (au[kAuWords * u + kAuFlags] & kAuKeyframe) {
      if (n_key++ == 0) first_key = u;
    }
  }

  // ---- ADTS frames, one walk per audio PES
  int64_t n_frames = 0;
  int rate = 0, chans = 0;
  const AudioSpan audio = audio_span(s);
  const uint8_t* A = s.es + audio.off;
  for (int64_t k = 0; k < audio.n_adts; ++k) {
    const ByteRange r = audio_pes_range(rows.audio, k, audio);
    const AdtsWalk w = adts_walk(A, r.start, r.end, k == 0, rate, chans);
    if (w.error) status |= kAdtsError;
    aframes[kApesWords * k + kApesFrames] = w.frames;
    aframes[kApesWords * k + kApesUsed] = w.used;
    n_frames += w.frames;
  }

  sinfo[kStatus] = status;
  sinfo[kNumNal] = n_nal;
  sinfo[kNumAu] = m;
  sinfo[kNumKeyframeAus] = n_key;
  sinfo[kFirstKeyframeAu] = first_key;
  sinfo[kNumAdtsFrames] = n_frames;
  sinfo[kAudioSampleRate] = rate;
  sinfo[kAudioChannels] = chans;
}

}  // namespace es
}  // namespace hlsp2p
