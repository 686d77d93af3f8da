// The sequential cbcs decryption of one demuxed segment over any reader (docs/CBCS.md), and the
// walk over a segment's protected samples that it shares with cenc (cenc_segment.hpp).
// runtime/cbcs.cpp runs it over a reader with a range test; tests/native/cbcs_main.cpp also over
// one without, under a sanitizer.  The senc, subsample, pattern and overlap rules are
// shared/grammar.hpp (namespace mp4), the same functions kernels/cbcs.hip calls.
#pragma once
#include <algorithm>
#include <cstring>
#include <vector>

#include "aes_host.hpp"
#include "cbcs.hpp"

namespace hlsp2p {
namespace mp4 {

// The senc entries of the recorded samples of the protected tracks, moof by moof, the overlap
// rule, then on_sample(t, k, entry, nsub, o, z) for every sample that is to be decrypted, the
// video track first (entry: where its senc entry lies; nsub < 0: no subsample table; o, z: its
// bytes).  false: no track is protected and nothing was walked.  status gains its no_senc /
// overlap / bad_senc bits, n_senc counts the senc boxes read.
// rd.u8(p) / rd.be32(p): byte p of the segment's n source bytes; asked only for bytes of [0, n).
template <class Reader, class OnSample>
bool protected_samples(Reader& rd, int64_t n, const CbcsDemux& md, const int64_t* prot, int64_t& status,
                       int64_t& n_senc, OnSample&& on_sample) {
  const int64_t max_pes = md.max_pes;
  const bool prot_on[kTracks] = {prot[kPrProtected] == 1, prot[kProtWords + kPrProtected] == 1};
  if (!prot_on[0] && !prot_on[1]) return false;
  const int64_t rec[kTracks] = {prot_on[0] ? clamp(md.minfo[kMTrack0 + kMtNumSamples], 0, max_pes) : 0,
                                prot_on[1] ? clamp(md.minfo[kMTrack0 + kMTrackWords + kMtNumSamples], 0, max_pes) : 0};
  const int64_t nr = clamp(md.minfo[kMNumRun], 0, md.max_run);
  const int iv_size[kTracks] = {iv_bytes(prot[kPrIvSize]), iv_bytes(prot[kProtWords + kPrIvSize])};
  int64_t tracks[kTracks * kTrackWords] = {};
  tracks[kTkId] = md.info[ts::kVideoPid];
  tracks[kTrackWords + kTkId] = md.info[ts::kAudioPid];
  struct Aux { int64_t entry, nsub, run; };
  std::vector<Aux> aux[kTracks];
  for (int t = 0; t < kTracks; ++t) aux[t].assign(static_cast<size_t>(rec[t]), Aux{-1, 0, -1});

  // ---- the senc entries of the recorded samples, moof by moof
  int64_t moof = 0, base = 0;
  top_walk(
      rd, n,
      [&](int64_t k, int64_t mp, const Box& mb) {
        if (k >= kMaxBoxRows) return;
        moof = k;
        while (base < nr && md.runs[base * kRunWords + kRnMoof] < moof) ++base;
        senc_walk(rd, mp, mb, tracks, n, [&](int slot, int64_t j0, int64_t cnt, int64_t sp, const Box& sb) {
          const int64_t g0 = base + j0;
          if (!prot_on[slot] || sp < 0 || g0 >= nr || md.runs[g0 * kRunWords + kRnMoof] != moof) return;
          ++n_senc;
          const SencHead h = senc_head(rd, sp, sb);
          if (!h.ok) {
            status |= kCbBadSenc;
            return;
          }
          int64_t e = 0, q = h.at;
          for (int64_t g = g0; g < g0 + cnt && g < nr; ++g) {
            const int64_t first = md.runs[g * kRunWords + kRnFirst], count = md.runs[g * kRunWords + kRnCount];
            for (int64_t j = 0; j < count; ++j, ++e) {
              const int64_t s = first + j;
              if (e >= h.count || s >= rec[slot]) return;
              int64_t nsub;
              const int64_t next = senc_entry(rd, q, h.end, iv_size[slot], (h.flags & 2) != 0, nsub);
              if (next < 0) {
                status |= kCbBadSenc;
                return;
              }
              aux[slot][static_cast<size_t>(s)] = Aux{q, nsub, g};
              q = next;
            }
          }
        });
      },
      [](int64_t, int64_t, const Box&) {});

  auto placed = [&](int t, int64_t k, int64_t& o, int64_t& z) {
    o = clamp(md.pes[table_words(t, max_pes, ts::kPesWords) + ts::kPesWords * k + ts::kPesEsOffset], 0, n);
    z = clamp(md.msamples[table_words(t, max_pes, kMsampleWords) + kMsampleWords * k + kMsSize], 0, n - o);
  };
  // ---- a run that shares bytes with a run in front of it stays encrypted
  std::vector<int64_t> lo(static_cast<size_t>(nr), int64_t(0x7fffffff)), hi(static_cast<size_t>(nr), int64_t(-1));
  for (int t = 0; t < kTracks; ++t)
    for (int64_t k = 0; k < rec[t]; ++k) {
      const Aux& ax = aux[t][static_cast<size_t>(k)];
      if (ax.entry < 0) continue;
      int64_t o, z;
      placed(t, k, o, z);
      if (z > 0) {
        lo[static_cast<size_t>(ax.run)] = std::min(lo[static_cast<size_t>(ax.run)], o);
        hi[static_cast<size_t>(ax.run)] = std::max(hi[static_cast<size_t>(ax.run)], o + z);
      }
    }
  std::vector<char> shadow(static_cast<size_t>(nr), 0);
  for (int64_t r = 0; r < nr; ++r)
    for (int64_t f = 0; f < r; ++f)
      if (spans_meet(lo[static_cast<size_t>(f)], hi[static_cast<size_t>(f)], lo[static_cast<size_t>(r)],
                     hi[static_cast<size_t>(r)]))
        shadow[static_cast<size_t>(r)] = 1;

  // ---- the samples in order, the video track first
  for (int t = 0; t < kTracks; ++t)
    for (int64_t k = 0; k < rec[t]; ++k) {
      const Aux& ax = aux[t][static_cast<size_t>(k)];
      if (ax.entry < 0) {
        status |= kCbNoSenc;
        continue;
      }
      if (shadow[static_cast<size_t>(ax.run)]) {
        status |= kCbOverlap;
        continue;
      }
      int64_t o, z;
      placed(t, k, o, z);
      on_sample(t, k, ax.entry, ax.nsub, o, z);
    }
  return true;
}

// The IV of a sample of track t whose senc entry lies at entry: its own, else the track's
// constant IV, else the job's; an 8-byte IV has zeros on the right.
template <class Reader>
void sample_iv(Reader& rd, const int64_t* prot, int t, int64_t entry, const uint8_t* const_iv, const uint8_t* iv,
               uint8_t out[es::kAesBlock]) {
  const int size = iv_bytes(prot[t * kProtWords + kPrIvSize]);
  std::memset(out, 0, es::kAesBlock);
  if (size > 0) {
    for (int i = 0; i < size; ++i) out[i] = static_cast<uint8_t>(rd.u8(entry + i));
  } else {
    std::memcpy(out, iv_bytes(prot[t * kProtWords + kPrConstIvSize]) > 0 ? const_iv + t * es::kAesBlock : iv,
                es::kAesBlock);
  }
}

// dst holds a copy of the n source bytes and gets the plaintext; the source is never written.
template <class Reader>
void cbcs_segment_with(Reader rd, int64_t n, const CbcsDemux& md, const int64_t* prot, const uint8_t* const_iv,
                       const uint8_t* iv, const uint32_t* drk, int64_t max_range, uint8_t* dst, int32_t* ranges,
                       int64_t* cinfo) {
  std::fill(ranges, ranges + table_words(1, max_range, kRangeWords), -1);
  std::fill(cinfo, cinfo + kCbInfoWords, int64_t(0));
  n = std::max<int64_t>(n, 0);
  int64_t status = (md.minfo[kMStatus] & kCbDamagedMask) ? kCbDemuxDamaged : 0;
  cinfo[kCbStatus] = status;
  const int iv_size[kTracks] = {iv_bytes(prot[kPrIvSize]), iv_bytes(prot[kProtWords + kPrIvSize])};
  int64_t n_ranges = 0, rank = 0, n_senc = 0;
  const bool any = protected_samples(rd, n, md, prot, status, n_senc,
                                     [&](int t, int64_t k, int64_t entry, int64_t nsub, int64_t o, int64_t z) {
    const int64_t c = prot[t * kProtWords + kPrCrypt], s = prot[t * kProtWords + kPrSkip];
    int64_t blocks = 0;
    const bool ok = sample_ranges(rd, o, z, entry + iv_size[t] + 2, nsub, [&](int64_t off, int64_t len) {
      const int64_t nb = cipher_blocks(len, c, s);
      if (nb <= 0) return;
      if (n_ranges < max_range) {
        int32_t* row = ranges + kRangeWords * n_ranges;
        row[kRgOffset] = static_cast<int32_t>(off);
        row[kRgLength] = static_cast<int32_t>(len);
        row[kRgSample] = static_cast<int32_t>((t << kRgTrackShift) | k);
        row[kRgRank] = static_cast<int32_t>(rank);
        uint8_t chain[es::kAesBlock];
        sample_iv(rd, prot, t, entry, const_iv, iv, chain);
        for (int64_t j = 0; j < nb; ++j) {
          const int64_t at = off + cipher_block_at(j, c, s);
          uint8_t cj[es::kAesBlock], p[es::kAesBlock];
          for (int i = 0; i < es::kAesBlock; ++i) cj[i] = static_cast<uint8_t>(rd.u8(at + i));
          aes::decrypt_block(drk, cj, p);
          for (int i = 0; i < es::kAesBlock; ++i) dst[at + i] = static_cast<uint8_t>(p[i] ^ chain[i]);
          std::memcpy(chain, cj, es::kAesBlock);
        }
      }
      ++n_ranges;
      rank += nb;
      blocks += nb;
    });
    if (!ok) status |= kCbBadSenc;
    if (blocks > 0) {
      cinfo[kCbVideoSamples + t] += 1;
      cinfo[kCbVideoBlocks + t] += blocks;
    }
  });
  if (!any) return;
  if (n_ranges > max_range) status |= kCbRangeOverflow;
  cinfo[kCbStatus] = status;
  cinfo[kCbNumRanges] = n_ranges;
  cinfo[kCbNumSenc] = n_senc;
}

}  // namespace mp4
}  // namespace hlsp2p
