// Stand-alone driver of the host AC-3 / E-AC-3 op for the sanitizer build of
// tests/test_ac3audio_native.py: reads a batch file and runs es::ac3_audio_segment on each segment
// with the segment's ES in a heap buffer of exactly cap bytes and its output region in one of
// exactly region bytes, so the sanitizer sees any byte read or written outside them.  Writes the
// six outputs.
//   in:  int64 B, max_pes, max_aframes, has_mpa; per segment int64 cap, region, then cap ES bytes, the
//        info row, the pes rows, the rinfo row, the asamples rows, the region's bytes as the ops in
//        front left them and, with has_mpa, the MPEG audio op's mpainfo row
//   out: per segment dframes, ac3info, mpainfo, asamples, rinfo, then the region's bytes
#include <cstdint>
#include <cstring>
#include <fstream>
#include <iterator>
#include <vector>

#include "ac3audio.hpp"

using namespace hlsp2p;

template <typename T>
static void put(std::ofstream& f, const std::vector<T>& v) {
  f.write(reinterpret_cast<const char*>(v.data()), static_cast<std::streamsize>(v.size() * sizeof(T)));
}

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  std::ifstream in(argv[1], std::ios::binary);
  const std::vector<char> raw((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
  size_t p = 0;
  auto i64 = [&]() {
    int64_t v;
    std::memcpy(&v, raw.data() + p, 8);
    p += 8;
    return v;
  };
  auto take = [&](auto& v) {
    if (v.empty()) return;
    std::memcpy(v.data(), raw.data() + p, v.size() * sizeof(v[0]));
    p += v.size() * sizeof(v[0]);
  };
  const int64_t B = i64(), max_pes = i64(), max_aframes = i64(), has_mpa = i64();
  std::ofstream out(argv[2], std::ios::binary);
  for (int64_t b = 0; b < B; ++b) {
    const int64_t cap = i64(), region = i64();
    std::vector<uint8_t> seg(static_cast<size_t>(cap));  // exactly cap bytes on the heap
    std::vector<int64_t> info(ts::kInfoWords), pes(ts::pes_words(1, max_pes)), rinfo(es::kRinfoWords),
        ac3info(es::kAc3infoWords), mpainfo(es::kMpainfoWords), mpa_in(has_mpa ? es::kMpainfoWords : 0);
    std::vector<int32_t> asamples(max_aframes * es::kAsampleWords), dframes(max_pes * es::kApesWords);
    std::vector<uint8_t> box(static_cast<size_t>(region));  // exactly region bytes on the heap
    take(seg), take(info), take(pes), take(rinfo), take(asamples), take(box), take(mpa_in);
    const int64_t off = 0;
    const es::Segment s = es::segment_at(seg.data(), &off, &cap, info.data(), pes.data(), max_pes, 0, 0);
    es::ac3_audio_segment(s, region, max_aframes,
                          {dframes.data(), ac3info.data(), mpainfo.data(), has_mpa ? mpa_in.data() : nullptr,
                           asamples.data(), rinfo.data()},
                          box.data());
    put(out, dframes), put(out, ac3info), put(out, mpainfo), put(out, asamples), put(out, rinfo), put(out, box);
  }
  return p == raw.size() ? 0 : 3;
}
