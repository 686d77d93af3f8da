// Host moof boxes: one sequential pass over the remux's sample rows.  The time rules and the words
// in front of the trun entries are shared/grammar.hpp (namespace es), the same functions
// kernels/fragment.hip calls.
#include "fragment.hpp"

namespace hlsp2p {
namespace es {

namespace {
void put_be32(uint8_t* p, uint32_t v) {
  p[0] = static_cast<uint8_t>(v >> 24);
  p[1] = static_cast<uint8_t>(v >> 16);
  p[2] = static_cast<uint8_t>(v >> 8);
  p[3] = static_cast<uint8_t>(v);
}
}  // namespace

void fragment_segment(const int64_t* rinfo, const int32_t* vsamples, const int32_t* asamples, int64_t rate,
                      const int64_t* fparam, int64_t max_pes, int64_t max_aframes, int64_t audio_gap, uint8_t* out,
                      int64_t* finfo, const int64_t* mpainfo) {
  const int64_t m = clamp(rinfo[kNumVsamples], 0, max_pes);
  const int64_t A0 = frag_audio_box(rinfo[kAudioBoxOffset], fparam[kFpRegion], audio_gap);
  int64_t n = 0;  // the recorded frames: rows with offset >= 0
  for (int64_t f = 0; f < max_aframes; ++f) n += asamples[kAsampleWords * f + kAsOffset] >= 0;
  const FragAudio fa = frag_audio(rate, mpainfo);
  const FragTimes ft = frag_times(m, rinfo[kVideoBaseDts], rinfo[kAudioBasePts], fa.rate, fparam[kFpTimeBase],
                                  fparam[kFpTimeRef], fparam[kFpAnchor] != 0);
  const uint32_t seq = static_cast<uint32_t>(fparam[kFpSequence]);
  const int64_t vbytes = moof_video_bytes(m), abytes = moof_audio_bytes(n);

  // ---- the video moof ends where the video mdat starts
  uint8_t* v = out - vbytes;
  for (int i = 0; i < kMoofVideoHead / 4; ++i)
    put_be32(v + 4 * i, moof_video_word(i, static_cast<uint32_t>(m), seq, static_cast<uint64_t>(ft.video_tfdt)));
  for (int64_t a = 0; a < m; ++a) {
    const int32_t* row = vsamples + a * kVsampleWords;
    uint8_t* e = v + kMoofVideoHead + kMoofVideoEntry * a;
    put_be32(e, static_cast<uint32_t>(row[kVsDuration]));
    put_be32(e + 4, static_cast<uint32_t>(row[kVsSize]));
    put_be32(e + 8, static_cast<uint32_t>(row[kVsFlags]));
    put_be32(e + 12, static_cast<uint32_t>(row[kVsCts]));
  }

  // ---- the audio moof ends where the audio mdat starts: the sizes of the first n rows
  uint8_t* a0 = out + A0 - abytes;
  for (int i = 0; i < kMoofAudioHead / 4; ++i)
    put_be32(a0 + 4 * i, moof_audio_word(i, static_cast<uint32_t>(n), seq, static_cast<uint64_t>(ft.audio_tfdt), fa.duration));
  for (int64_t f = 0; f < n; ++f)
    put_be32(a0 + kMoofAudioHead + kMoofAudioEntry * f, static_cast<uint32_t>(asamples[kAsampleWords * f + kAsSize]));

  finfo[kFStatus] = ft.status;
  finfo[kFVideoMoofBytes] = vbytes;
  finfo[kFAudioMoofBytes] = abytes;
  finfo[kFVideoTfdt] = ft.video_tfdt;
  finfo[kFAudioTfdt] = ft.audio_tfdt;
  finfo[kFTimeBase] = ft.base;
  finfo[kFNumAsamples] = n;
  finfo[kFSpare] = 0;
}

}  // namespace es
}  // namespace hlsp2p
