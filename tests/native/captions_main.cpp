// Stand-alone driver of the host caption extraction (runtime/captions.cpp caption_segment) for
// tests/test_captions_native.py, which builds it with -fsanitize=address,undefined.
// Input file, little-endian: int64 B, max_pes, max_nal, max_cc; then per segment int64 cap, cap
// bytes of ES, and the rows info (int64), pes (int64), nal, au, aframes (int32) and sinfo (int64) at
// their layout.hpp sizes.
// Output file: per segment ccsamples, ccpts, ccbytes, cc608 and ccinfo, and the cap bytes of ES as
// they are after the call.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "captions.hpp"

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
  const int64_t B = head[0], max_pes = head[1], max_nal = head[2], max_cc = head[3];
  if (!es::max_cc_ok(max_cc)) return 3;
  for (int64_t b = 0; b < B; ++b) {
    std::vector<int64_t> cap, info, pes, sinfo;
    std::vector<uint8_t> es;
    std::vector<int32_t> nal, au, aframes;
    if (!read_vec(f, cap, 1) || !read_vec(f, es, static_cast<size_t>(cap[0])) || !read_vec(f, info, ts::kInfoWords) ||
        !read_vec(f, pes, static_cast<size_t>(ts::pes_words(1, max_pes))) ||
        !read_vec(f, nal, static_cast<size_t>(table_words(1, max_nal, es::kNalWords))) ||
        !read_vec(f, au, static_cast<size_t>(table_words(1, max_pes, es::kAuWords))) ||
        !read_vec(f, aframes, static_cast<size_t>(table_words(1, max_pes, es::kApesWords))) ||
        !read_vec(f, sinfo, es::kSinfoWords))
      return 3;
    std::vector<int32_t> samples(static_cast<size_t>(max_cc * es::kCcRowWords), 7);
    std::vector<int64_t> pts(static_cast<size_t>(max_cc), 7), ccinfo(es::kCcInfoWords, 7);
    std::vector<uint8_t> bytes(static_cast<size_t>(max_cc * es::kCcSlotBytes), 7);
    std::vector<uint8_t> cc608(static_cast<size_t>(max_cc * 2 * es::kCcFieldBytes), 7);
    const es::Segment s{es.data(), cap[0], info.data(), pes.data(), max_pes, max_nal};
    const es::IndexTables<const int32_t, const int64_t> ix{nal.data(), au.data(), aframes.data(), sinfo.data()};
    es::caption_segment(s, ix, true, max_cc, {samples.data(), pts.data(), bytes.data(), cc608.data(), ccinfo.data()});
    write_vec(o, samples);
    write_vec(o, pts);
    write_vec(o, bytes);
    write_vec(o, cc608);
    write_vec(o, ccinfo);
    write_vec(o, es);
  }
  std::fclose(f);
  return std::fclose(o) == 0 ? 0 : 4;
}
