// Host remux: one sequential pass over the index rows.  The keep rule, the ADTS frame rule and
// the timestamp differences are shared/grammar.hpp (namespace es), the same functions
// kernels/remux.hip calls.
#include "remux.hpp"

#include <algorithm>
#include <cstring>

#include "grammar.hpp"

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

void remux_segment(const uint8_t* es, int64_t cap, const int64_t* info, const int64_t* pes, int64_t max_pes,
                   int64_t max_nal, const int32_t* nal, const int32_t* au, const int32_t* aframes,
                   const int64_t* sinfo, int64_t max_aframes, int32_t* vsamples, int32_t* asamples, int64_t* rinfo,
                   uint8_t* out) {
  std::fill(vsamples, vsamples + max_pes * kVsampleWords, -1);
  std::fill(asamples, asamples + max_aframes * kAsampleWords, -1);
  cap = std::max<int64_t>(cap, 0);
  const int64_t vtype = info[ts::kVideoType];
  const bool supported = video_supported(vtype);
  const bool hevc = is_hevc(vtype);
  int64_t status = supported ? 0 : kRemuxUnsupportedVideo;
  if (sinfo[kStatus] & kNalOverflow) status |= kTruncated;
  const int64_t R = supported ? clamp(sinfo[kNumNal], 0, max_nal) : 0;
  const int64_t m = supported ? clamp(sinfo[kNumAu], 0, max_pes) : 0;
  const int64_t* vp = pes;                // class 0
  const int64_t* ap = pes + max_pes * 3;  // class 1
  const int64_t region = remux_out_bytes(cap, max_nal);
  const int64_t v_limit = remux_video_limit(cap, max_nal);

  // ---- sample rows: timestamps and flags; sizes follow from the NAL rows
  for (int64_t a = 0; a < m; ++a) {
    int32_t* row = vsamples + a * kVsampleWords;
    Delta32 dur = {0, true};
    if (a + 1 < m) dur = delta32(vp[3 * (a + 1) + 2], vp[3 * a + 2], true);
    else if (m > 1) dur = delta32(vp[3 * a + 2], vp[3 * (a - 1) + 2], true);
    const Delta32 cts = delta32(vp[3 * a + 1], vp[3 * a + 2], false);
    if (!dur.fits || !cts.fits) status |= kBadTimestamps;
    row[0] = 0;
    row[1] = 0;
    row[2] = dur.v;
    row[3] = cts.v;
    row[4] = (au[4 * a + 2] & kAuKeyframe) ? kSampleSync : kSampleNonSync;
  }

  // ---- video payload: a 4-byte length, then the NAL's bytes
  uint8_t* vout = out + 8;
  int64_t P = 0;
  bool fit = true;
  for (int64_t k = 0; k < R; ++k) {
    const int64_t s = clamp(nal[4 * k], 0, cap);
    const int64_t len = clamp(nal[4 * k + 1], 0, cap - s);
    const int64_t a = nal[4 * k + 3];
    if (a < 0 || a >= m || len <= 0 || !nal_kept(hevc, nal[4 * k + 2])) continue;
    if (fit && P + 4 + len > v_limit) {  // possible with damaged rows only
      fit = false;
      status |= kTruncated;
    }
    if (!fit) continue;
    vout[P] = static_cast<uint8_t>(len >> 24);
    vout[P + 1] = static_cast<uint8_t>(len >> 16);
    vout[P + 2] = static_cast<uint8_t>(len >> 8);
    vout[P + 3] = static_cast<uint8_t>(len);
    std::memcpy(vout + P + 4, es + s, static_cast<size_t>(len));
    vsamples[a * kVsampleWords + 1] += static_cast<int32_t>(4 + len);
    P += 4 + len;
  }
  int64_t off = 0;
  for (int64_t a = 0; a < m; ++a) {
    vsamples[a * kVsampleWords] = static_cast<int32_t>(off);
    off += vsamples[a * kVsampleWords + 1];
  }
  box_header(out, 8 + P);

  // ---- audio payload: the counted ADTS frames without their headers
  const int64_t A0 = (8 + P + 15) & ~int64_t(15);
  const int64_t room = region - (A0 + 8);
  const int64_t ma = clamp(info[ts::kNumAudioPes], 0, max_pes);
  int64_t Q = 0, n_rec = 0, n_frames = 0;
  if (is_adts(info[ts::kAudioType])) {
    const int64_t a_off = clamp(info[ts::kAudioEsOffset], 0, cap);
    const int64_t a_len = clamp(info[ts::kAudioBytes], 0, cap - a_off);
    const uint8_t* A = es + a_off;
    uint8_t* aout = out + A0 + 8;
    bool open = true;
    for (int64_t k = 0; k < ma; ++k) {
      const int64_t start = clamp(ap[3 * k], 0, a_len);
      const int64_t end = k + 1 < ma ? clamp(ap[3 * (k + 1)], start, a_len) : a_len;
      const int64_t want = aframes[2 * k];
      int64_t q = start;
      for (int64_t j = 0; j < want; ++j) {
        const AdtsFrame f = adts_frame_at(A, q, end);
        if (f.len == 0) break;
        const int64_t size = f.len - f.hdr;
        ++n_frames;
        if (open && n_rec < max_aframes && Q + size <= room) {
          asamples[2 * n_rec] = static_cast<int32_t>(Q);
          asamples[2 * n_rec + 1] = static_cast<int32_t>(size);
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
  }
  box_header(out + A0, 8 + Q);

  rinfo[kRStatus] = status;
  rinfo[kVideoPayloadBytes] = P;
  rinfo[kNumVsamples] = m;
  rinfo[kAudioBoxOffset] = A0;
  rinfo[kAudioPayloadBytes] = Q;
  rinfo[kNumAframes] = n_frames;
  rinfo[kVideoBaseDts] = m > 0 ? vp[2] : -1;
  rinfo[kAudioBasePts] = ma > 0 ? ap[1] : -1;
}

}  // namespace es
}  // namespace hlsp2p
