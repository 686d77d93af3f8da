// The sequential cenc decryption of one demuxed segment over any reader (docs/CENC.md), on the
// walk of cbcs_segment.hpp.  runtime/cenc.cpp runs it over a reader with a range test;
// tests/native/cenc_main.cpp also over one without, under a sanitizer.  The range, unit and counter
// rules are shared/grammar.hpp (namespace mp4), the same functions kernels/cenc.hip calls.
#pragma once
#include "cbcs_segment.hpp"
#include "cenc.hpp"

namespace hlsp2p {
namespace mp4 {

template <class Reader>
void cenc_segment_with(Reader rd, int64_t n, const CbcsDemux& md, const int64_t* prot, const uint8_t* const_iv,
                       const uint8_t* iv, const uint32_t* erk, int64_t max_range, uint8_t* dst, int32_t* ranges,
                       int64_t* cinfo) {
  std::fill(ranges, ranges + table_words(1, max_range, kCnRangeWords), -1);
  std::fill(cinfo, cinfo + kCnInfoWords, int64_t(0));
  n = std::max<int64_t>(n, 0);
  int64_t status = (md.minfo[kMStatus] & kCbDamagedMask) ? kCbDemuxDamaged : 0;
  cinfo[kCnStatus] = status;
  const int iv_size[kTracks] = {iv_bytes(prot[kPrIvSize]), iv_bytes(prot[kProtWords + kPrIvSize])};
  int64_t n_ranges = 0, rank = 0, n_senc = 0;
  const bool any = protected_samples(rd, n, md, prot, status, n_senc,
                                     [&](int t, int64_t k, int64_t entry, int64_t nsub, int64_t o, int64_t z) {
    int64_t p0 = 0;  // protected bytes of the sample so far
    const bool ok = sample_ranges(rd, o, z, entry + iv_size[t] + 2, nsub, [&](int64_t off, int64_t len) {
      const int64_t u = ctr_units(p0, len);
      if (u <= 0) return;
      if (n_ranges < max_range) {
        int32_t* row = ranges + kCnRangeWords * n_ranges;
        row[kCnOffset] = static_cast<int32_t>(off);
        row[kCnLength] = static_cast<int32_t>(len);
        row[kCnSample] = static_cast<int32_t>((t << kRgTrackShift) | k);
        row[kCnRank] = static_cast<int32_t>(rank);
        row[kCnStreamPos] = static_cast<int32_t>(p0);
        row[kCnIvOffset] = static_cast<int32_t>(iv_size[t] > 0 ? entry : -1);
        row[kCnSpare0] = row[kCnSpare1] = 0;
        uint8_t ivb[es::kAesBlock];
        sample_iv(rd, prot, t, entry, const_iv, iv, ivb);
        uint32_t ivw[4];
        for (int w = 0; w < 4; ++w)
          ivw[w] = static_cast<uint32_t>(ivb[4 * w]) | (static_cast<uint32_t>(ivb[4 * w + 1]) << 8) |
                   (static_cast<uint32_t>(ivb[4 * w + 2]) << 16) | (static_cast<uint32_t>(ivb[4 * w + 3]) << 24);
        for (int64_t m = 0; m < u; ++m) {
          const int64_t j = ctr_unit_block(p0, m), at = ctr_block_at(off, p0, j);
          uint32_t cw[4];
          ctr_block(ivw, j, cw);
          uint8_t ctr[es::kAesBlock], ks[es::kAesBlock];
          for (int i = 0; i < es::kAesBlock; ++i) ctr[i] = static_cast<uint8_t>(cw[i >> 2] >> (8 * (i & 3)));
          aes::encrypt_block(erk, ctr, ks);
          const int64_t lo = std::max(at, off), hi = std::min(at + es::kAesBlock, off + len);
          for (int64_t f = lo; f < hi; ++f) dst[f] = static_cast<uint8_t>(rd.u8(f) ^ ks[f - at]);
        }
      }
      ++n_ranges;
      rank += u;
      p0 += len;
    });
    if (!ok) status |= kCbBadSenc;
    if (p0 > 0) {
      cinfo[kCnVideoSamples + t] += 1;
      cinfo[kCnVideoBytes + t] += p0;
    }
  });
  if (!any) return;
  if (n_ranges > max_range) status |= kCbRangeOverflow;
  cinfo[kCnStatus] = status;
  cinfo[kCnNumRanges] = n_ranges;
  cinfo[kCnNumSenc] = n_senc;
  cinfo[kCnNumUnits] = rank;
}

}  // namespace mp4
}  // namespace hlsp2p
