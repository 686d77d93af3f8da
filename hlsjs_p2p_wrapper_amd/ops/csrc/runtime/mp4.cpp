// Host fragmented-MP4 demux: mp4_segment.hpp's sequential passes over a reader that answers a byte
// outside the segment with 0, so a broken rule could not read memory.
#include "mp4.hpp"

#include "mp4_segment.hpp"

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

void demux_segment(const uint8_t* S, int64_t n, const int64_t* tracks, const Limits& lim, const Tables& out) {
  demux_segment_with(HostReader{S, std::max<int64_t>(n, 0)}, n, tracks, lim, out);
}

}  // namespace mp4
}  // namespace hlsp2p
