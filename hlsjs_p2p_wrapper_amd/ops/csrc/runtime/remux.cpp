// Host remux: one sequential pass over the index rows.  The segment view, the keep rule, the ADTS
// frame rule and the timestamp differences are shared/grammar.hpp (namespace es), the same
// functions kernels/remux.hip calls.
#include "remux.hpp"

#include <algorithm>
#include <cstring>

namespace hlsp2p {
namespace es {

namespace {
void box_header(uint8_t* p, int64_t size) {
  p[0] = static_cast<uint8_t>(size >> 24);
  p[1] = static_cast<uint8_t>(size >> 16);
  p[2] = static_cast<uint8_t>(size >> 8);
  p[3] = static_cast<uint8_t>(size);
  std::memcpy(p + 4, "mdat", 4);
}
}  // namespace

void remux_segment(Segment s, const IndexTables<const int32_t, const int64_t>& ix, int64_t max_aframes,
                   const RemuxTables& t, uint8_t* out, int64_t audio_gap) {
  const int64_t max_pes = s.max_pes, max_nal = s.max_nal;
  const int32_t *nal = ix.nal, *au = ix.au, *aframes = ix.aframes;
  int32_t *vsamples = t.vsamples, *asamples = t.asamples;
  std::fill(vsamples, vsamples + table_words(1, max_pes, kVsampleWords), -1);
  std::fill(asamples, asamples + table_words(1, max_aframes, kAsampleWords), -1);
  s.cap = std::max<int64_t>(s.cap, 0);  // the host takes any cap: a negative one reads nothing
  const int64_t cap = s.cap;
  const uint8_t* es = s.es;
  const VideoSpan video = video_span(s);
  const bool hevc = video.hevc;
  int64_t status = video.supported ? 0 : kRemuxUnsupportedVideo;
  if (ix.sinfo[kStatus] & kNalOverflow) status |= kTruncated;
  const int64_t R = video_rows(video, ix.sinfo[kNumNal], max_nal);
  const int64_t m = video_rows(video, ix.sinfo[kNumAu], max_pes);  // the index's count, not the demux's
  const PesRows rows = pes_rows(s);
  const int64_t *vp = rows.video, *ap = rows.audio;
  const int64_t region = remux_out_bytes(cap, max_nal) + audio_gap;
  const int64_t v_limit = remux_video_limit(cap, max_nal);

  // ---- sample rows: timestamps and flags; sizes follow from the NAL rows
  for (int64_t a = 0; a < m; ++a) {
    int32_t* row = vsamples + a * kVsampleWords;
    Delta32 dur = {0, true};
    if (a + 1 < m) dur = delta32(pes_at(vp, a + 1, ts::kPesDts), pes_at(vp, a, ts::kPesDts), true);
    else if (m > 1) dur = delta32(pes_at(vp, a, ts::kPesDts), pes_at(vp, a - 1, ts::kPesDts), true);
    const Delta32 cts = delta32(pes_at(vp, a, ts::kPesPts), pes_at(vp, a, ts::kPesDts), false);
    if (!dur.fits || !cts.fits) status |= kBadTimestamps;
    row[kVsOffset] = 0;
    row[kVsSize] = 0;
    row[kVsDuration] = dur.v;
    row[kVsCts] = cts.v;
    row[kVsFlags] = (au[kAuWords * a + kAuFlags] & kAuKeyframe) ? kSampleSync : kSampleNonSync;
  }

  // ---- video payload: a 4-byte length, then the NAL's bytes
  uint8_t* vout = out + 8;
  int64_t P = 0;
  bool fit = true;
  for (int64_t k = 0; k < R; ++k) {
    const int32_t* row = nal + kNalWords * k;
    const int64_t b = clamp(row[kNalOffset], 0, cap);
    const int64_t len = clamp(row[kNalLength], 0, cap - b);
    const int64_t a = row[kNalAu];
    if (a < 0 || a >= m || len <= 0 || !nal_kept(hevc, row[kNalType])) continue;
    if (fit && P + 4 + len > v_limit) {  // possible with damaged rows only
      fit = false;
      status |= kTruncated;
    }
    if (!fit) continue;
    vout[P] = static_cast<uint8_t>(len >> 24);
    vout[P + 1] = static_cast<uint8_t>(len >> 16);
    vout[P + 2] = static_cast<uint8_t>(len >> 8);
    vout[P + 3] = static_cast<uint8_t>(len);
    std::memcpy(vout + P + 4, es + b, static_cast<size_t>(len));
    vsamples[a * kVsampleWords + kVsSize] += static_cast<int32_t>(4 + len);
    P += 4 + len;
  }
  int64_t off = 0;
  for (int64_t a = 0; a < m; ++a) {
    vsamples[a * kVsampleWords + kVsOffset] = static_cast<int32_t>(off);
    off += vsamples[a * kVsampleWords + kVsSize];
  }
  box_header(out, 8 + P);

  // ---- audio payload: the counted ADTS frames without their headers
  const int64_t A0 = audio_box_offset(P, audio_gap);
  const int64_t room = region - (A0 + 8);
  const AudioSpan audio = audio_span(s);
  int64_t Q = 0, n_rec = 0, n_frames = 0;
  const uint8_t* A = es + audio.off;
  uint8_t* aout = out + A0 + 8;
  bool open = true;
  for (int64_t k = 0; k < audio.n_adts; ++k) {
    const ByteRange r = audio_pes_range(ap, k, audio);
    const int64_t start = r.start, end = r.end;
    const int64_t want = aframes[kApesWords * k + kApesFrames];
    int64_t q = start;
    for (int64_t j = 0; j < want; ++j) {
      const AdtsFrame f = adts_frame_at(A, q, end);
      if (f.len == 0) break;
      const int64_t size = f.len - f.hdr;
      ++n_frames;
      if (open && n_rec < max_aframes && Q + size <= room) {
        asamples[kAsampleWords * n_rec + kAsOffset] = static_cast<int32_t>(Q);
        asamples[kAsampleWords * n_rec + kAsSize] = static_cast<int32_t>(size);
        std::memcpy(aout + Q, A + q + f.hdr, static_cast<size_t>(size));
        Q += size;
        ++n_rec;
      } else {
        open = false;
        status |= kAframeOverflow;
      }
      q += f.len;
    }
  }
  box_header(out + A0, 8 + Q);

  int64_t* rinfo = t.rinfo;
  rinfo[kRStatus] = status;
  rinfo[kVideoPayloadBytes] = P;
  rinfo[kNumVsamples] = m;
  rinfo[kAudioBoxOffset] = A0;
  rinfo[kAudioPayloadBytes] = Q;
  rinfo[kNumAframes] = n_frames;
  rinfo[kVideoBaseDts] = m > 0 ? pes_at(vp, 0, ts::kPesDts) : -1;
  rinfo[kAudioBasePts] = audio.n_pes > 0 ? pes_at(ap, 0, ts::kPesPts) : -1;
}

}  // namespace es
}  // namespace hlsp2p
