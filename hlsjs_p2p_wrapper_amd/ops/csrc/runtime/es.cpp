// Host sample index: the serial loops that fill the rows.  The codec, NAL-type and ADTS byte
// rules are shared/grammar.hpp (namespace es), the same functions kernels/es_index.hip calls.
#include "es.hpp"

#include <algorithm>
#include <vector>

#include "grammar.hpp"
#include "ts.hpp"

namespace hlsp2p {
namespace es {

void index_segment(const uint8_t* es, int64_t cap, const int64_t* info, const int64_t* pes, int64_t max_pes,
                   int64_t max_nal, int32_t* nal, int32_t* au, int32_t* aframes, int64_t* sinfo) {
  std::fill(nal, nal + max_nal * 4, -1);
  std::fill(au, au + max_pes * 4, -1);
  std::fill(aframes, aframes + max_pes * 2, -1);
  std::fill(sinfo, sinfo + kSinfoWords, int64_t(0));
  sinfo[kFirstKeyframeAu] = -1;
  cap = std::max<int64_t>(cap, 0);
  const int64_t vtype = info[ts::kVideoType];
  const bool supported = video_supported(vtype);
  const bool hevc = is_hevc(vtype);
  int64_t status = supported ? 0 : kUnsupportedVideo;
  const uint8_t* V = es;
  const int64_t n = supported ? clamp(info[ts::kVideoBytes], 0, cap) : 0;

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
  const int64_t m = supported ? clamp(info[ts::kNumVideoPes], 0, max_pes) : 0;  // unsupported: no units either
  const int64_t* vp = pes;  // class 0
  int64_t a = -1;           // access unit of the current NAL: PES offsets ascend with the NAL starts
  for (int64_t k = 0; k < nn; ++k) {
    const int64_t s = p[k] + 3;
    int64_t e = n;
    if (k + 1 < n_nal) {
      const int64_t p1 = p[k + 1];
      const int64_t z1 = (p1 > 0 && V[p1 - 1] == 0) ? 1 : 0;
      e = std::max(s, p1 - z1);
    }
    while (a + 1 < m && vp[3 * (a + 1)] <= s) ++a;
    nal[4 * k] = static_cast<int32_t>(s);
    nal[4 * k + 1] = static_cast<int32_t>(e - s);
    nal[4 * k + 2] = e == s ? -1 : nal_type(hevc, V[s]);
    nal[4 * k + 3] = static_cast<int32_t>(a);
  }

  // ---- access unit rows
  int64_t n_key = 0, first_key = -1;
  for (int64_t u = 0; u < m; ++u) {
    const int64_t next = u + 1 < m ? vp[3 * (u + 1)] : n;
    au[4 * u] = -1;
    au[4 * u + 1] = 0;
    au[4 * u + 2] = 0;
    au[4 * u + 3] = static_cast<int32_t>(next - vp[3 * u]);
  }
  for (int64_t k = 0; k < nn; ++k) {
    const int64_t u = nal[4 * k + 3];
    if (u < 0) continue;
    if (au[4 * u + 1] == 0) au[4 * u] = static_cast<int32_t>(k);
    ++au[4 * u + 1];
    au[4 * u + 2] |= nal_flags(hevc, nal[4 * k + 2]);
  }
  for (int64_t u = 0; u < m; ++u) {
    if (au[4 * u + 2] & kAuKeyframe) {
      if (n_key++ == 0) first_key = u;
    }
  }

  // ---- ADTS frames, one walk per audio PES
  int64_t n_frames = 0;
  int rate = 0, chans = 0;
  if (is_adts(info[ts::kAudioType])) {
    const int64_t a_off = clamp(info[ts::kAudioEsOffset], 0, cap);
    const int64_t a_len = clamp(info[ts::kAudioBytes], 0, cap - a_off);
    const uint8_t* A = es + a_off;
    const int64_t ma = clamp(info[ts::kNumAudioPes], 0, max_pes);
    const int64_t* ap = pes + max_pes * 3;  // class 1
    for (int64_t k = 0; k < ma; ++k) {
      const int64_t start = clamp(ap[3 * k], 0, a_len);
      const int64_t end = k + 1 < ma ? clamp(ap[3 * (k + 1)], start, a_len) : a_len;
      const AdtsWalk w = adts_walk(A, start, end, k == 0, rate, chans);
      if (w.error) status |= kAdtsError;
      aframes[2 * k] = w.frames;
      aframes[2 * k + 1] = w.used;
      n_frames += w.frames;
    }
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
