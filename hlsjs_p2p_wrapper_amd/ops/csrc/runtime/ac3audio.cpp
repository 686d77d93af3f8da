// Host AC-3 / E-AC-3 audio: one sequential pass over the audio PES rows.  The header rule, the PES
// range and the walk are shared/grammar.hpp (namespace es), the same functions kernels/ac3_audio.hip
// calls.
#include "ac3audio.hpp"

#include <algorithm>
#include <cstring>

namespace hlsp2p {
namespace es {

void ac3_audio_segment(Segment s, int64_t region, int64_t max_aframes, const Ac3Tables& t, uint8_t* out) {
  std::fill(t.dframes, t.dframes + table_words(1, s.max_pes, kApesWords), -1);
  std::fill(t.ac3info, t.ac3info + kAc3infoWords, int64_t(0));
  std::fill(t.mpainfo, t.mpainfo + kMpainfoWords, int64_t(0));
  if (!is_dolby_audio(s.info[ts::kAudioType])) {
    t.ac3info[kAcStatus] = kAc3NotDolbyAudio;
    if (t.mpa_in) std::copy(t.mpa_in, t.mpa_in + kMpainfoWords, t.mpainfo);
    else t.mpainfo[kMpStatus] = kMpaNotMpegAudio;
    return;
  }
  s.cap = std::max<int64_t>(s.cap, 0);  // the host takes any cap: a negative one reads nothing
  const AudioSpan audio = audio_span(s);
  const int64_t* ap = pes_rows(s).audio;
  const uint8_t* A = s.es + audio.off;
  const auto frame_at = [A](int64_t q, int64_t end) { return ac3_frame_at(A, q, end); };
  Ac3Frame first = ac3_frame_at(A, 0, 0);
  if (audio.n_pes > 0) {
    const ByteRange r0 = mpa_pes_range(ap, 0, audio);
    first = frame_at(r0.start, r0.end);
  }
  if (!first.counts) {
    t.ac3info[kAcStatus] = kAc3NoAudioConfig | (first.len > 0 && !first.layout_ok ? kAc3UnsupportedLayout : 0);
    t.mpainfo[kMpStatus] = kMpaNoAudioConfig;
    return;
  }
  const int64_t A0 = mpa_audio_box(t.rinfo[kAudioBoxOffset], region);
  const int64_t room = region - (A0 + 8);
  uint8_t* aout = out + A0 + 8;
  int64_t status = 0, Q = 0, n_rec = 0, n_frames = 0;
  bool open = true;
  for (int64_t k = 0; k < audio.n_pes; ++k) {
    const ByteRange r = mpa_pes_range(ap, k, audio);
    const MpaWalk w = mpa_walk(frame_at, r.start, r.end, first.key, [&](int32_t, int64_t q, int32_t len) {
      ++n_frames;
      if (open && n_rec < max_aframes && Q + len <= room) {
        t.asamples[kAsampleWords * n_rec + kAsOffset] = static_cast<int32_t>(Q);
        t.asamples[kAsampleWords * n_rec + kAsSize] = len;
        std::memcpy(aout + Q, A + q, static_cast<size_t>(len));
        Q += len;
        ++n_rec;
      } else {
        open = false;
        status |= kAc3AframeOverflow;
      }
    });
    if (w.error) status |= kAc3Error;
    if (w.format_change) status |= kAc3FormatChange;
    t.dframes[kApesWords * k + kApesFrames] = w.frames;
    t.dframes[kApesWords * k + kApesUsed] = w.used;
  }
  if (region >= A0 + 8) {
    const uint32_t size = static_cast<uint32_t>(8 + Q);
    out[A0] = static_cast<uint8_t>(size >> 24);
    out[A0 + 1] = static_cast<uint8_t>(size >> 16);
    out[A0 + 2] = static_cast<uint8_t>(size >> 8);
    out[A0 + 3] = static_cast<uint8_t>(size);
    std::memcpy(out + A0 + 4, "mdat", 4);
  }
  t.rinfo[kAudioPayloadBytes] = Q;
  t.rinfo[kNumAframes] = n_frames;
  if (status & kAc3AframeOverflow) t.rinfo[kRStatus] |= kAframeOverflow;
  ac3_info_row(t.ac3info, status, n_frames, first);
  ac3_mpainfo_row(t.mpainfo, n_frames, first);
}

}  // namespace es
}  // namespace hlsp2p
