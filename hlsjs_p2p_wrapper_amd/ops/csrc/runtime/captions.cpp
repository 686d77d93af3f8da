// Host caption extraction: one sequential pass over the NAL rows, a byte-by-byte unescape of each
// candidate's stored bytes and the shared message walk.  The segment view, the candidate test, the
// emulation-prevention predicate, cc_find and the 608 pair rule are shared/grammar.hpp (namespace
// es), the same functions kernels/captions.hip calls.
#include "captions.hpp"

#include <algorithm>
#include <cstring>

namespace hlsp2p {
namespace es {

void caption_segment(Segment s, const IndexTables<const int32_t, const int64_t>& ix, bool enable, int64_t max_cc,
                     const CcTables& out) {
  std::fill(out.samples, out.samples + max_cc * kCcRowWords, -1);
  std::fill(out.pts, out.pts + max_cc, int64_t(-1));
  std::memset(out.bytes, 0, static_cast<size_t>(max_cc * kCcSlotBytes));
  std::memset(out.cc608, 0, static_cast<size_t>(max_cc * 2 * kCcFieldBytes));
  std::fill(out.info, out.info + kCcInfoWords, 0);
  if (!enable) return;
  s.cap = std::max<int64_t>(s.cap, 0);  // the host takes any cap: a negative one reads nothing
  const int64_t cap = s.cap;
  const VideoSpan video = video_span(s);
  const int64_t R = video_rows(video, ix.sinfo[kNumNal], s.max_nal);
  const int64_t m = video_rows(video, ix.sinfo[kNumAu], s.max_pes);
  const int h = nal_header_bytes(video.hevc);
  const int64_t* vp = pes_rows(s).video;
  int64_t status = cc_status(s, ix.sinfo);
  int64_t n_sei = 0, total = 0, rec = 0;
  uint8_t U[kCcNalBytes];

  for (int64_t k = 0; k < R; ++k) {
    const int32_t* row = ix.nal + kNalWords * k;
    const int64_t off = clamp(row[kNalOffset], 0, cap);
    const int64_t n = clamp(row[kNalLength], 0, cap - off);
    const int64_t au = row[kNalAu];
    if (!cc_nal_candidate(video.hevc, row[kNalType], au, m, n)) continue;
    ++n_sei;
    if (n > kCcNalBytes) status |= kCcSeiClipped;
    const int stored = static_cast<int>(std::min<int64_t>(n, kCcNalBytes));
    const uint8_t* b = s.es + off;
    int u = 0;
    for (int j = h; j < stored; ++j)
      if (j < 2 || !is_emulation_prevention(b[j - 2], b[j - 1], b[j])) U[u++] = b[j];
    const uint8_t* up = U;
    const CcMatch hit = cc_find([up](int i) { return static_cast<int>(up[i]); }, u);
    if (hit.count < 0) continue;
    if (total++ >= max_cc) continue;
    const int64_t r = rec++;
    const int size = 2 + 3 * hit.count;
    uint8_t* dst = out.bytes + r * kCcSlotBytes;
    std::memcpy(dst, U + hit.at, static_cast<size_t>(size));
    uint8_t* f608 = out.cc608 + r * 2 * kCcFieldBytes;
    int pairs[2] = {0, 0};
    for (int t = 0; t < hit.count; ++t) {
      const int f = dst[2 + 3 * t], b1 = dst[3 + 3 * t], b2 = dst[4 + 3 * t];
      const int field = cc_608_field(f, b1, b2);
      if (field < 0) continue;
      f608[field * kCcFieldBytes + 2 * pairs[field]] = static_cast<uint8_t>(b1 & 0x7f);
      f608[field * kCcFieldBytes + 2 * pairs[field] + 1] = static_cast<uint8_t>(b2 & 0x7f);
      ++pairs[field];
    }
    int32_t* sr = out.samples + kCcRowWords * r;
    sr[kCrNal] = static_cast<int32_t>(k);
    sr[kCrAu] = static_cast<int32_t>(au);
    sr[kCrSize] = size;
    sr[kCrCount] = hit.count;
    sr[kCrOrder] = 0;
    sr[kCrField1Pairs] = pairs[0];
    sr[kCrField2Pairs] = pairs[1];
    sr[kCrFlags] = (dst[0] & 0x40) ? kCcProcess : 0;
    out.pts[r] = pes_at(vp, au, ts::kPesPts);
    out.info[kCiNumTriples] += hit.count;
    out.info[kCiField1Pairs] += pairs[0];
    out.info[kCiField2Pairs] += pairs[1];
  }
  if (total > max_cc) status |= kCcOverflow;
  int64_t first = -1, last = -1;
  for (int64_t r = 0; r < rec; ++r) {
    const int64_t p = out.pts[r];
    int32_t order = 0;
    for (int64_t q = 0; q < rec; ++q) order += out.pts[q] < p || (out.pts[q] == p && q < r);
    out.samples[kCcRowWords * r + kCrOrder] = order;
    first = r == 0 ? p : std::min(first, p);
    last = r == 0 ? p : std::max(last, p);
  }
  out.info[kCiStatus] = status;
  out.info[kCiNumSei] = n_sei;
  out.info[kCiNumSamples] = total;
  out.info[kCiFirstPts] = first;
  out.info[kCiLastPts] = last;
}

}  // namespace es
}  // namespace hlsp2p
