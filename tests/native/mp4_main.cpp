// Stand-alone driver of the host fragmented-MP4 demux for the sanitizer build of
// tests/test_mp4demux_native.py: reads a batch file, runs mp4::demux_segment (the shipped reader) on
// each segment with the segment's bytes in a heap buffer of exactly n bytes, and the same passes
// (mp4::demux_segment_with) over a reader of its own that has no range test, so the sanitizer would
// see a rule that asked for a byte outside the segment; the two results must agree (exit code 4).
// Writes the ten tables and the bytes.
//   in:  int64 B, max_pes, max_nal, max_moof, max_run, max_emsg; per segment int64 n, int64 tracks[16], n bytes
//   out: per segment minfo, msamples, runs, emsg, info, pes, nal, au, aframes, sinfo, then the n bytes
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>
#include <vector>

#include "mp4.hpp"
#include "mp4_segment.hpp"

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
  const int64_t B = i64();
  mp4::Limits lim;
  lim.max_pes = i64(), lim.max_nal = i64(), lim.max_moof = i64(), lim.max_run = i64(), lim.max_emsg = i64();
  std::ofstream out(argv[2], std::ios::binary);
  for (int64_t b = 0; b < B; ++b) {
    const int64_t n = i64();
    int64_t tracks[mp4::kTracks * mp4::kTrackWords];
    for (int64_t& t : tracks) t = i64();
    std::vector<uint8_t> seg(raw.begin() + p, raw.begin() + p + n);  // exactly n bytes on the heap
    p += static_cast<size_t>(n);
    std::vector<int64_t> minfo(mp4::kMinfoWords), runs(lim.max_run * mp4::kRunWords), emsg(lim.max_emsg * mp4::kEmsgWords),
        info(ts::kInfoWords), pes(ts::pes_words(1, lim.max_pes)), sinfo(es::kSinfoWords);
    std::vector<int32_t> msamples(mp4::kTracks * lim.max_pes * mp4::kMsampleWords), nal(lim.max_nal * es::kNalWords),
        au(lim.max_pes * es::kAuWords), aframes(lim.max_pes * es::kApesWords);
    const mp4::Tables t{minfo.data(), msamples.data(), runs.data(), emsg.data(), info.data(), pes.data(),
                        {nal.data(), au.data(), aframes.data(), sinfo.data()}};
    mp4::demux_segment(seg.data(), n, tracks, lim, t);
    auto minfo2 = minfo, runs2 = runs, emsg2 = emsg, info2 = info, pes2 = pes, sinfo2 = sinfo;
    auto msamples2 = msamples, nal2 = nal, au2 = au, aframes2 = aframes;
    const mp4::Tables t2{minfo2.data(), msamples2.data(), runs2.data(), emsg2.data(), info2.data(), pes2.data(),
                         {nal2.data(), au2.data(), aframes2.data(), sinfo2.data()}};
    mp4::demux_segment_with(RawReader{seg.data()}, n, tracks, lim, t2);
    if (!(same(minfo, minfo2) && same(msamples, msamples2) && same(runs, runs2) && same(emsg, emsg2) &&
          same(info, info2) && same(pes, pes2) && same(nal, nal2) && same(au, au2) && same(aframes, aframes2) &&
          same(sinfo, sinfo2)))
      return 4;
    put(out, minfo), put(out, msamples), put(out, runs), put(out, emsg), put(out, info), put(out, pes);
    put(out, nal), put(out, au), put(out, aframes), put(out, sinfo), put(out, seg);
  }
  return p == raw.size() ? 0 : 3;
}
