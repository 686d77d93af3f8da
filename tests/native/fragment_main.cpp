// Stand-alone driver of the host moof writer (runtime/fragment.cpp fragment_segment) for
// tests/test_fragment_native.py, which builds it with -fsanitize=address,undefined.
// Input file, little-endian: int64 B, max_pes, max_aframes, audio_gap; then per segment the rows
// rinfo (int64), vsamples, asamples (int32) at their layout.hpp sizes, int64 rate, the fparams row
// (int64), and frag_headroom(max_pes) + fparams[kFpRegion] bytes: the segment's headroom and
// region as the remux left them.
// Output file: per segment the finfo row and the same bytes as they are after the call.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "fragment.hpp"

using namespace hlsp2p;

template <typename T>
static bool read_vec(std::FILE* f, std::vector<T>& v, size_t n) {
  v.resize(n);  // an exact-size heap buffer: an access one element outside is the sanitizer's to report
  return n == 0 || std::fread(v.data(), sizeof(T), n, f) == n;
}
template <typename T>
static void write_vec(std::FILE* f, const std::vector<T>& v) {
  if (!v.empty()) std::fwrite(v.data(), sizeof(T), v.size(), f);
}

int main(int argc, char** argv) {
  if (argc != 3) {
    std::fprintf(stderr, "usage: %s batch.bin out.bin\n", argv[0]);
    return 2;
  }
  std::FILE* f = std::fopen(argv[1], "rb");
  std::FILE* o = std::fopen(argv[2], "wb");
  if (!f || !o) return 2;
  std::vector<int64_t> head;
  if (!read_vec(f, head, 4)) return 3;
  const int64_t B = head[0], max_pes = head[1], max_aframes = head[2], audio_gap = head[3];
  if (max_pes <= 0 || max_aframes <= 0 || audio_gap < es::frag_audio_gap(max_aframes) || audio_gap % 16) return 3;
  const int64_t headroom = es::frag_headroom(max_pes);
  for (int64_t b = 0; b < B; ++b) {
    std::vector<int64_t> rinfo, rate, fparam;
    std::vector<int32_t> vsamples, asamples;
    std::vector<uint8_t> bytes;
    if (!read_vec(f, rinfo, es::kRinfoWords) ||
        !read_vec(f, vsamples, static_cast<size_t>(table_words(1, max_pes, es::kVsampleWords))) ||
        !read_vec(f, asamples, static_cast<size_t>(table_words(1, max_aframes, es::kAsampleWords))) ||
        !read_vec(f, rate, 1) || !read_vec(f, fparam, es::kFparamWords))
      return 3;
    const int64_t region = fparam[es::kFpRegion];
    if (region < audio_gap + 32 || !read_vec(f, bytes, static_cast<size_t>(headroom + region))) return 3;
    std::vector<int64_t> finfo(es::kFinfoWords, 7);
    es::fragment_segment(rinfo.data(), vsamples.data(), asamples.data(), rate[0], fparam.data(), max_pes, max_aframes,
                         audio_gap, bytes.data() + headroom, finfo.data());
    write_vec(o, finfo);
    write_vec(o, bytes);
  }
  std::fclose(f);
  return std::fclose(o) == 0 ? 0 : 4;
}
