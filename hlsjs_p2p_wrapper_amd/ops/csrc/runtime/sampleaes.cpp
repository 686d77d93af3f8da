// Host SAMPLE-AES decryption: one sequential pass over the NAL rows and one over the audio PES.
// The segment view, the candidate / protected / cipher-block rules and the ADTS frame rule are
// shared/grammar.hpp (namespace es), the same functions kernels/sample_aes.hip calls.
#include "sampleaes.hpp"

#include <algorithm>
#include <cstring>

#include "aes_host.hpp"

namespace hlsp2p {
namespace es {

namespace {
// P = D(C) xor chain, and the chain moves on to C: dst may be C itself
void cbc_block(const uint32_t* drk, uint8_t chain[kAesBlock], uint8_t* c) {
  uint8_t keep[kAesBlock], p[kAesBlock];
  std::memcpy(keep, c, kAesBlock);
  aes::decrypt_block(drk, c, p);
  for (int i = 0; i < kAesBlock; ++i) c[i] = static_cast<uint8_t>(p[i] ^ chain[i]);
  std::memcpy(chain, keep, kAesBlock);
}
}  // namespace

void sample_decrypt_segment(Segment s, uint8_t* es, const IndexTables<int32_t, const int64_t>& ix,
                            const uint32_t drk[kAesRoundKeyWords], const uint8_t iv[kAesBlock], int64_t* sainfo) {
  s.cap = std::max<int64_t>(s.cap, 0);  // the host takes any cap: a negative one touches nothing
  const int64_t cap = s.cap;
  std::fill(sainfo, sainfo + kSaWords, 0);
  sainfo[kSaStatus] = sample_status(s, ix.sinfo);
  uint8_t chain[kAesBlock];

  // ---- video: H.264 only
  const VideoSpan video = video_span(s);
  if (s.info[ts::kVideoType] == ts::kAvc) {
    const int64_t R = video_rows(video, ix.sinfo[kNumNal], s.max_nal);
    const int64_t m = video_rows(video, ix.sinfo[kNumAu], s.max_pes);
    for (int64_t k = 0; k < R; ++k) {
      int32_t* row = ix.nal + kNalWords * k;
      const int64_t off = clamp(row[kNalOffset], 0, cap);
      const int64_t n = clamp(row[kNalLength], 0, cap - off);
      if (!sample_nal_candidate(row[kNalType], row[kNalAu], m, n)) continue;
      uint8_t* b = es + off;
      // the unescaped length first: a candidate that is not protected keeps its bytes
      int64_t u = 0;
      for (int64_t j = 0; j < n; ++j)
        if (j < 2 || !is_emulation_prevention(b[j - 2], b[j - 1], b[j])) ++u;
      if (!sample_nal_protected(u)) continue;
      // compaction towards lower addresses; p2 / p1 are the raw predecessors, read before the
      // write position can reach them
      int64_t w = 0;
      int p2 = -1, p1 = -1;
      for (int64_t j = 0; j < n; ++j) {
        const int c = b[j];
        if (j < 2 || !is_emulation_prevention(p2, p1, c)) b[w++] = static_cast<uint8_t>(c);
        p2 = p1;
        p1 = c;
      }
      std::memset(b + u, 0, static_cast<size_t>(n - u));
      std::memcpy(chain, iv, kAesBlock);
      const int64_t blocks = sample_video_blocks(u);
      for (int64_t j = 0; j < blocks; ++j) cbc_block(drk, chain, b + sample_block_at(j));
      row[kNalLength] = static_cast<int32_t>(u);
      sainfo[kSaProtectedNals] += 1;
      sainfo[kSaRemovedBytes] += n - u;
      sainfo[kSaVideoBlocks] += blocks;
    }
  }

  // ---- audio: the counted ADTS frames, walked as the remux walks them
  const AudioSpan audio = audio_span(s);
  const int64_t* ap = pes_rows(s).audio;
  uint8_t* A = es + audio.off;
  for (int64_t k = 0; k < audio.n_adts; ++k) {
    const ByteRange r = audio_pes_range(ap, k, audio);
    const int64_t want = ix.aframes[kApesWords * k + kApesFrames];
    int64_t q = r.start;
    for (int64_t j = 0; j < want; ++j) {
      const AdtsFrame f = adts_frame_at(A, q, r.end);
      if (f.len == 0) break;
      const int64_t nb = sample_audio_blocks(f);
      std::memcpy(chain, iv, kAesBlock);
      for (int64_t i = 0; i < nb; ++i) cbc_block(drk, chain, A + q + f.hdr + kSaAudioLead + kAesBlock * i);
      if (nb > 0) {
        sainfo[kSaAudioFrames] += 1;
        sainfo[kSaAudioBlocks] += nb;
      }
      q += f.len;
    }
  }
}

}  // namespace es
}  // namespace hlsp2p
