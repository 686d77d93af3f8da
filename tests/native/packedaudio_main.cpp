// Stand-alone driver of the host packed-audio demux for the sanitizer build of
// tests/test_packedaudio_native.py: reads a batch file, runs es::packed_segment (the shipped reader)
// on each segment with the segment's bytes in a heap buffer of exactly cap bytes, and the same
// passes (es::packed_segment_with) over a reader of its own that has no range test, so the sanitizer
// would see a rule that asked for a byte outside the segment; the two results must agree (exit
// code 4).  Writes the seven tables and the bytes.
//   in:  int64 B, max_pes; per segment int64 n, n bytes
//   out: per segment info, pes, nal, au, aframes, sinfo, painfo, then the n bytes
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>
#include <vector>

#include "packedaudio.hpp"

using namespace hlsp2p;

struct RawReader {
  const uint8_t* S;
  int u8(int64_t p) const { return S[p]; }
  uint32_t be32(int64_t p) const { return mp4::be32_bytes(*this, p); }
};

template <typename T>
static bool same(const std::vector<T>& a, const std::vector<T>& b) {
  return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0);
}

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
  const int64_t B = i64(), max_pes = i64();
  std::ofstream out(argv[2], std::ios::binary);
  for (int64_t b = 0; b < B; ++b) {
    const int64_t n = i64();
    std::vector<uint8_t> seg(raw.begin() + p, raw.begin() + p + n);  // exactly n bytes on the heap
    p += static_cast<size_t>(n);
    std::vector<int64_t> info(ts::kInfoWords), pes(ts::pes_words(1, max_pes)), sinfo(es::kSinfoWords),
        painfo(es::kPainfoWords);
    std::vector<int32_t> nal(es::kPackedNalRows * es::kNalWords), au(max_pes * es::kAuWords),
        aframes(max_pes * es::kApesWords);
    const es::PackedTables t{info.data(), pes.data(), {nal.data(), au.data(), aframes.data(), sinfo.data()},
                             painfo.data()};
    es::packed_segment(seg.data(), n, max_pes, t);
    auto info2 = info, pes2 = pes, sinfo2 = sinfo, painfo2 = painfo;
    auto nal2 = nal, au2 = au, aframes2 = aframes;
    const es::PackedTables t2{info2.data(), pes2.data(), {nal2.data(), au2.data(), aframes2.data(), sinfo2.data()},
                              painfo2.data()};
    es::packed_segment_with(RawReader{seg.data()}, seg.data(), n, max_pes, t2);
    if (!(same(info, info2) && same(pes, pes2) && same(nal, nal2) && same(au, au2) && same(aframes, aframes2) &&
          same(sinfo, sinfo2) && same(painfo, painfo2)))
      return 4;
    put(out, info), put(out, pes), put(out, nal), put(out, au), put(out, aframes), put(out, sinfo), put(out, painfo);
    put(out, seg);
  }
  return p == raw.size() ? 0 : 3;
}
