// Stand-alone driver of the host cenc decrypt for the sanitizer build of tests/test_cenc_native.py:
// reads a batch file, demuxes each segment (mp4::demux_segment) and runs mp4::cenc_segment (the
// shipped reader) on it with the segment's bytes and the copy in heap buffers of exactly n bytes, and
// the same pass (mp4::cenc_segment_with) over a reader of its own that has no range test, so the
// sanitizer would see a rule that asked for a byte outside the segment; the two results must agree
// (exit code 4).  Writes ranges, cinfo, the copy and the source bytes.
//   in:  int64 B, max_pes, max_nal, max_moof, max_run, max_emsg, max_range; per segment int64 n,
//        int64 tracks[16], int64 prot[16], 32 constant-IV bytes, 16 IV bytes, 16 key bytes, n bytes
//   out: per segment ranges, cinfo, the n bytes of the copy, the n source bytes
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>
#include <vector>

#include "aes_host.hpp"
#include "cenc.hpp"
#include "cenc_segment.hpp"
#include "mp4.hpp"

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
  auto bytes = [&](size_t n) {
    std::vector<uint8_t> v(raw.begin() + p, raw.begin() + p + n);
    p += n;
    return v;
  };
  const int64_t B = i64();
  mp4::Limits lim;
  lim.max_pes = i64(), lim.max_nal = i64(), lim.max_moof = i64(), lim.max_run = i64(), lim.max_emsg = i64();
  const int64_t max_range = i64();
  std::ofstream out(argv[2], std::ios::binary);
  for (int64_t b = 0; b < B; ++b) {
    const int64_t n = i64();
    int64_t tracks[mp4::kTracks * mp4::kTrackWords], prot[mp4::kTracks * mp4::kProtWords];
    for (int64_t& t : tracks) t = i64();
    for (int64_t& t : prot) t = i64();
    const std::vector<uint8_t> civ = bytes(mp4::kTracks * es::kAesBlock), iv = bytes(es::kAesBlock), key = bytes(16);
    const std::vector<uint8_t> seg = bytes(static_cast<size_t>(n));  // exactly n bytes on the heap
    uint32_t erk[es::kAesRoundKeyWords];
    aes::expand_key_enc(key.data(), erk);
    std::vector<int64_t> minfo(mp4::kMinfoWords), runs(lim.max_run * mp4::kRunWords), emsg(lim.max_emsg * mp4::kEmsgWords),
        info(ts::kInfoWords), pes(ts::pes_words(1, lim.max_pes)), sinfo(es::kSinfoWords);
    std::vector<int32_t> msamples(mp4::kTracks * lim.max_pes * mp4::kMsampleWords), nal(lim.max_nal * es::kNalWords),
        au(lim.max_pes * es::kAuWords), aframes(lim.max_pes * es::kApesWords);
    const mp4::Tables t{minfo.data(), msamples.data(), runs.data(), emsg.data(), info.data(), pes.data(),
                        {nal.data(), au.data(), aframes.data(), sinfo.data()}};
    mp4::demux_segment(seg.data(), n, tracks, lim, t);
    const mp4::CbcsDemux md{minfo.data(), runs.data(), info.data(), pes.data(), msamples.data(), lim.max_pes, lim.max_run};
    std::vector<uint8_t> copy(seg), copy2(seg);
    std::vector<int32_t> ranges(max_range * mp4::kCnRangeWords), ranges2(ranges);
    std::vector<int64_t> cinfo(mp4::kCnInfoWords), cinfo2(cinfo);
    mp4::cenc_segment(seg.data(), n, md, prot, civ.data(), iv.data(), erk, max_range, copy.data(), ranges.data(),
                      cinfo.data());
    mp4::cenc_segment_with(RawReader{seg.data()}, n, md, prot, civ.data(), iv.data(), erk, max_range, copy2.data(),
                           ranges2.data(), cinfo2.data());
    if (!(same(copy, copy2) && same(ranges, ranges2) && same(cinfo, cinfo2))) return 4;
    put(out, ranges), put(out, cinfo), put(out, copy), put(out, seg);
  }
  return p == raw.size() ? 0 : 3;
}
