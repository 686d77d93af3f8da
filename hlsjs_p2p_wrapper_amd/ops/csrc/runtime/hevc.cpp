// Host HEVC configuration: one sequential pass over the NAL rows, a byte-by-byte unescape and the
// shared parser.  The segment view, the emulation-prevention predicate and hevc_sps_parse are
// shared/grammar.hpp (namespace es), the same functions kernels/hevc_config.hip calls.
#include "hevc.hpp"

#include <algorithm>
#include <cstring>
#include <vector>

namespace hlsp2p {
namespace es {

HevcSpsRow parse_hevc_sps_nal(const uint8_t* b, int64_t n) {
  std::vector<uint8_t> rbsp;
  rbsp.reserve(static_cast<size_t>(std::max<int64_t>(n, 1)));
  for (int64_t j = kHevcNalHeader; j < n; ++j)
    if (!is_emulation_prevention(b[j - 2], b[j - 1], b[j])) rbsp.push_back(b[j]);
  HevcSpsRow r;
  r.rbsp_bytes = static_cast<int32_t>(rbsp.size());
  const uint8_t* p = rbsp.data();
  r.ok = hevc_sps_parse([p](int64_t i) { return p[i]; }, static_cast<int64_t>(rbsp.size()), r.f);
  return r;
}

void hevc_config_segment(Segment s, const IndexTables<const int32_t, const int64_t>& ix, int64_t max_ps, uint8_t* hps,
                         int32_t* hinfo) {
  std::memset(hps, 0, static_cast<size_t>(hps_bytes(1, max_ps)));
  std::fill(hinfo, hinfo + kHinfoWords, 0);
  static constexpr int kNalSlot[kHpsRows] = {kHVpsNal, kHSpsNal, kHPpsNal};
  static constexpr int kBytesSlot[kHpsRows] = {kHVpsBytes, kHSpsBytes, kHPpsBytes};
  static constexpr int kType[kHpsRows] = {kHevcVps, kHevcSps, kHevcPps};
  static constexpr int32_t kMissing[kHpsRows] = {kHNoVps, kHNoSps, kHNoPps};
  for (int which = 0; which < kHpsRows; ++which) hinfo[kNalSlot[which]] = -1;
  if (!is_hevc(s.info[ts::kVideoType])) {  // nothing is searched or stored
    hinfo[kHStatus] = kHNotHevc;
    return;
  }
  s.cap = std::max<int64_t>(s.cap, 0);  // the host takes any cap: a negative one reads nothing
  const int64_t cap = s.cap;
  int32_t status = 0;

  // ---- the first non-empty VPS, SPS and PPS rows
  const int64_t R = video_rows(video_span(s), ix.sinfo[kNumNal], s.max_nal);
  int64_t found[kHpsRows] = {-1, -1, -1};
  for (int64_t k = 0; k < R && (found[kHpsVps] < 0 || found[kHpsSps] < 0 || found[kHpsPps] < 0); ++k) {
    const int32_t* row = ix.nal + kNalWords * k;
    if (row[kNalLength] <= 0) continue;
    for (int which = 0; which < kHpsRows; ++which)
      if (row[kNalType] == kType[which] && found[which] < 0) found[which] = k;
  }
  for (int which = 0; which < kHpsRows; ++which) {
    const int64_t k = found[which];
    if (k < 0) {
      status |= kMissing[which];
      continue;
    }
    const int32_t* row = ix.nal + kNalWords * k;
    const int64_t b = clamp(row[kNalOffset], 0, cap);
    const int64_t len = clamp(row[kNalLength], 0, cap - b);
    const int64_t stored = std::min(len, max_ps);
    uint8_t* dst = hps + which * max_ps;
    std::memcpy(dst, s.es + b, static_cast<size_t>(stored));
    if (len > max_ps) status |= kHPsOverflow;
    hinfo[kNalSlot[which]] = static_cast<int32_t>(k);
    hinfo[kBytesSlot[which]] = static_cast<int32_t>(len);
    if (which == kHpsSps && len <= max_ps) {  // an overflowed SPS is not parsed
      const HevcSpsRow r = parse_hevc_sps_nal(dst, len);
      if (!r.ok) status |= kHBadSps;
      hinfo[kHSpsRbspBytes] = r.rbsp_bytes;
      std::memcpy(hinfo + kHProfileSpace, &r.f, sizeof r.f);
    }
  }
  hinfo[kHStatus] = status;
}

}  // namespace es
}  // namespace hlsp2p
