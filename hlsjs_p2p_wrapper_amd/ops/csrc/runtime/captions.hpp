// CEA-608/708 caption data of one demuxed and indexed segment (docs/CAPTIONS.md holds the rules):
// every SEI NAL unit of an access unit is unescaped and its messages walked; the first ATSC A/53
// 'GA94' caption payload of a NAL becomes a sample with its access unit's pts, its 608 byte pairs
// split by field and its presentation rank.  The sequential host implementation;
// kernels/captions.hip reproduces its output exactly.
#pragma once
#include <cstdint>

#include "grammar.hpp"

namespace hlsp2p {
namespace es {

// row layouts (CcRow, Ccinfo), status bits (CcStatus) and the slot sizes: shared/layout.hpp

// segment b of a batch's tables (CcTables: shared/layout.hpp)
inline CcTables cc_tables_at(const CcTables& t, int64_t max_cc, int64_t b) {
  return {t.samples + table_words(b, max_cc, kCcRowWords), t.pts + b * max_cc, t.bytes + b * max_cc * kCcSlotBytes,
          t.cc608 + b * max_cc * 2 * kCcFieldBytes, t.info + b * kCcInfoWords};
}

// One segment.
//   s:      as index_segment took it; the ES is only read
//   ix:     what index_segment wrote (rows are used as found, clamped)
//   enable: false: the fill values and an all-zero info row
//   max_cc: max_cc_ok(max_cc)
void caption_segment(Segment s, const IndexTables<const int32_t, const int64_t>& ix, bool enable, int64_t max_cc,
                     const CcTables& out);

}  // namespace es
}  // namespace hlsp2p
