// Host packed-audio demux: packedaudio.hpp's sequential passes over a reader that answers a byte
// outside the segment with 0, so a broken rule could not read memory.
#include "packedaudio.hpp"

namespace hlsp2p {
namespace es {

namespace {
struct HostReader {
  const uint8_t* S;
  int64_t n;
  int u8(int64_t p) const { return p >= 0 && p < n ? S[p] : 0; }
  uint32_t be32(int64_t p) const { return mp4::be32_bytes(*this, p); }
};
}  // namespace

void packed_segment(const uint8_t* S, int64_t n, int64_t max_pes, const PackedTables& out) {
  n = std::max<int64_t>(n, 0);
  packed_segment_with(HostReader{S, n}, S, n, max_pes, out);
}

}  // namespace es
}  // namespace hlsp2p
