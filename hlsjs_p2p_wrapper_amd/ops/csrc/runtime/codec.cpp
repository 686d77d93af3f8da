// Host codec configuration: one sequential pass over the NAL rows, a byte-by-byte unescape and
// the shared parser.  The segment view, the emulation-prevention predicate, sps_parse and the
// ADTS fields are shared/grammar.hpp (namespace es), the same functions kernels/codec_config.hip
// calls.
#include "codec.hpp"

#include <algorithm>
#include <cstring>
#include <vector>

namespace hlsp2p {
namespace es {

SpsRow parse_sps_nal(const uint8_t* b, int64_t n) {
  std::vector<uint8_t> rbsp;
  rbsp.reserve(static_cast<size_t>(std::max<int64_t>(n, 1)));
  for (int64_t j = 1; j < n; ++j)
    if (j < 2 || !is_emulation_prevention(b[j - 2], b[j - 1], b[j])) rbsp.push_back(b[j]);
  SpsRow r;
  r.rbsp_bytes = static_cast<int32_t>(rbsp.size());
  const uint8_t* p = rbsp.data();
  r.ok = sps_parse([p](int64_t i) { return p[i]; }, static_cast<int64_t>(rbsp.size()), r.f);
  return r;
}

void config_segment(Segment s, const IndexTables<const int32_t, const int64_t>& ix, int64_t max_ps, uint8_t* ps,
                    int32_t* cinfo) {
  std::memset(ps, 0, static_cast<size_t>(ps_bytes(1, max_ps)));
  std::fill(cinfo, cinfo + kCinfoWords, 0);
  cinfo[kCSpsNal] = cinfo[kCPpsNal] = -1;
  s.cap = std::max<int64_t>(s.cap, 0);  // the host takes any cap: a negative one reads nothing
  const int64_t cap = s.cap;
  int32_t status = 0;

  // ---- parameter sets: the first non-empty SPS and PPS rows, H.264 only
  if (s.info[ts::kVideoType] != ts::kAvc) {
    status |= kConfigUnsupportedVideo;
  } else {
    const int64_t R = video_rows(video_span(s), ix.sinfo[kNumNal], s.max_nal);
    int64_t found[kPsRows] = {-1, -1};
    for (int64_t k = 0; k < R && (found[kPsSps] < 0 || found[kPsPps] < 0); ++k) {
      const int32_t* row = ix.nal + kNalWords * k;
      if (row[kNalLength] <= 0) continue;
      const int which = row[kNalType] == 7 ? kPsSps : row[kNalType] == 8 ? kPsPps : -1;
      if (which >= 0 && found[which] < 0) found[which] = k;
    }
    for (int which = 0; which < kPsRows; ++which) {
      const int64_t k = found[which];
      if (k < 0) {
        status |= which == kPsSps ? kNoSps : kNoPps;
        continue;
      }
      const int32_t* row = ix.nal + kNalWords * k;
      const int64_t b = clamp(row[kNalOffset], 0, cap);
      const int64_t len = clamp(row[kNalLength], 0, cap - b);
      const int64_t stored = std::min(len, max_ps);
      uint8_t* dst = ps + which * max_ps;
      std::memcpy(dst, s.es + b, static_cast<size_t>(stored));
      if (len > max_ps) status |= kPsOverflow;
      cinfo[which == kPsSps ? kCSpsNal : kCPpsNal] = static_cast<int32_t>(k);
      cinfo[which == kPsSps ? kCSpsBytes : kCPpsBytes] = static_cast<int32_t>(len);
      if (which == kPsSps && len <= max_ps) {  // an overflowed SPS is not parsed
        const SpsRow r = parse_sps_nal(dst, len);
        if (!r.ok) status |= kBadSps;
        cinfo[kCSpsRbspBytes] = r.rbsp_bytes;
        std::memcpy(cinfo + kCProfileIdc, &r.f, sizeof r.f);
      }
    }
  }

  // ---- audio: the ADTS header the index took the sample rate from
  const AudioSpan audio = audio_span(s);
  bool usable = false;
  if (audio.n_adts >= 1 && ix.aframes[kApesFrames] >= 1) {
    const ByteRange r = audio_pes_range(pes_rows(s).audio, 0, audio);
    if (r.start + 7 <= r.end) {
      const AdtsConfig c = adts_config_at(s.es + audio.off, r.start);
      cinfo[kCAacObjectType] = c.object_type;
      cinfo[kCAacRateIndex] = c.rate_index;
      cinfo[kCAacChannelConfig] = c.channel_config;
      usable = adts_config_usable(c);
    }
  }
  if (!usable) status |= kNoAudioConfig;
  cinfo[kCStatus] = status;
}

}  // namespace es
}  // namespace hlsp2p
