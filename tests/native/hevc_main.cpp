// Stand-alone driver of the host HEVC SPS parser (runtime/hevc.cpp parse_hevc_sps_nal) for
// tests/test_hevcconfig_native.py, which builds it with -fsanitize=address,undefined.
// Input file: per blob a little-endian uint32 length, then that many bytes of one SPS NAL unit.
// Output: one line per blob, "ok rbsp_bytes" and the fourteen HevcSpsFields in hinfo order.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "hevc.hpp"

int main(int argc, char** argv) {
  if (argc != 2) {
    std::fprintf(stderr, "usage: %s blobs.bin\n", argv[0]);
    return 2;
  }
  std::FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  unsigned char hdr[4];
  while (std::fread(hdr, 1, 4, f) == 4) {
    const uint32_t n = hdr[0] | (hdr[1] << 8) | (hdr[2] << 16) | (uint32_t(hdr[3]) << 24);
    // an exact-size heap buffer: a read one byte past the blob is the sanitizer's to report
    std::vector<uint8_t> blob(n);
    if (n && std::fread(blob.data(), 1, n, f) != n) return 3;
    const hlsp2p::es::HevcSpsRow r = hlsp2p::es::parse_hevc_sps_nal(blob.data(), n);
    const hlsp2p::es::HevcSpsFields& s = r.f;
    std::printf("%d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d\n", r.ok ? 1 : 0, r.rbsp_bytes, s.profile_space,
                s.tier_flag, s.profile_idc, s.profile_compat, s.constraint_hi, s.constraint_lo, s.level_idc,
                s.num_temporal_layers, s.temporal_id_nested, s.chroma_format_idc, s.bit_depth_luma,
                s.bit_depth_chroma, s.width, s.height);
  }
  std::fclose(f);
  return 0;
}
