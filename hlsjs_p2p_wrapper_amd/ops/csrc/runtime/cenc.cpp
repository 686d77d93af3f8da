// Host cenc decryption: cenc_segment.hpp's sequential pass over a reader that answers a byte
// outside the segment with 0, so a broken rule could not read memory.
#include "cenc.hpp"

#include "cenc_segment.hpp"

namespace hlsp2p {
namespace mp4 {

namespace {
struct HostReader {
  const uint8_t* S;
  int64_t n;
  int u8(int64_t p) const { return p >= 0 && p < n ? S[p] : 0; }
  uint32_t be32(int64_t p) const { return be32_bytes(*this, p); }
};
}  // namespace

void cenc_segment(const uint8_t* S, int64_t n, const CbcsDemux& md, const int64_t* prot, const uint8_t* const_iv,
                  const uint8_t* iv, const uint32_t* erk, int64_t max_range, uint8_t* dst, int32_t* ranges,
                  int64_t* cinfo) {
  cenc_segment_with(HostReader{S, std::max<int64_t>(n, 0)}, n, md, prot, const_iv, iv, erk, max_range, dst, ranges,
                    cinfo);
}

}  // namespace mp4
}  // namespace hlsp2p
