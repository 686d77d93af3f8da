// Row layouts, status bits, tile geometry and workspace sizes: the only definition of each, for
// the host runtime, the gfx950 kernels and their bindings.  <cstdint> only, constexpr.
#pragma once
#include <cstdint>

namespace hlsp2p {

// ---------------------------------------------------------------- MPEG-TS demux
namespace ts {
constexpr int kPacket = 188;
constexpr int kPsiScanPackets = 64;  // PAT/PMT must appear within the first 64 packets
constexpr int kClasses = 3;          // 0 video, 1 audio, 2 id3/metadata
constexpr int kInfoWords = 24;
constexpr int kBlockPackets = 256;   // packets per demux block (one lane each)

// info[] row (int64), identical on host and device; per-class families are base + class
enum Info : int {
  kStatus = 0,
  kPmtPid = 1,
  kVideoPid = 2, kAudioPid = 3, kId3Pid = 4,
  kNumPackets = 5,
  kVideoBytes = 6, kAudioBytes = 7, kId3Bytes = 8,
  kNumVideoPes = 9, kNumAudioPes = 10, kNumId3Pes = 11,
  kVideoType = 12, kAudioType = 13,
  kPayloadBytes = 14,   // total ES bytes (video+audio+id3)
  kFirstPts = 16,       // kFirstPts + class: PTS of the class's first PES (-1 if none)
  kLastPts = 19,        // kLastPts + class: PTS of the class's last PES
  kAudioEsOffset = 22,  // byte offset of the audio ES from the segment's ES start (video at 0)
  kId3EsOffset = 23,    // byte offset of the id3 ES: [video | audio | id3] packed back to back
};
enum Status : int64_t { kBadSync = 1, kNoPat = 2, kNoPmt = 4, kPesOverflow = 8, kPesHeaderError = 16, kBadLength = 32 };

// demux blocks of a segment of at most n bytes
constexpr int64_t demux_blocks(int64_t n) { return ((n + kPacket - 1) / kPacket + kBlockPackets - 1) / kBlockPackets; }
// 16-byte packet-header records the decrypt writes for an encrypted segment of n bytes
constexpr int64_t header_records(int64_t n) { return n / kPacket + 2; }

// aux workspace (int32), element offsets:
// [blk_sums: blocks x 2 x classes | blk_pre: the same | seg_tot: nseg x 2 x classes | spare: nseg]
struct DemuxAux { int64_t blk_sums, blk_pre, seg_tot, end; };
constexpr DemuxAux demux_aux(int64_t total_blocks, int64_t nseg) {
  return {0, total_blocks * 2 * kClasses, total_blocks * 4 * kClasses,
          total_blocks * 4 * kClasses + nseg * (2 * kClasses + 1)};
}
// elements of the three demux workspaces: meta (int32), pts_dts (int64), aux (int32)
struct DemuxWorkspace { int64_t meta, pts_dts, aux; };
constexpr DemuxWorkspace demux_workspace(int64_t total_blocks, int64_t nseg) {
  return {total_blocks * kBlockPackets, total_blocks * kBlockPackets * 2, demux_aux(total_blocks, nseg).end};
}
}  // namespace ts

// ---------------------------------------------------------------- sample index
namespace es {
constexpr int kSinfoWords = 8;
constexpr int64_t kDefaultMaxNal = 2048;

// sinfo[] row (int64), identical on host and device
enum Sinfo : int {
  kStatus = 0,
  kNumNal = 1,  // true total, also when the table overflowed
  kNumAu = 2, kNumKeyframeAus = 3,
  kFirstKeyframeAu = 4,  // -1: none
  kNumAdtsFrames = 5, kAudioSampleRate = 6, kAudioChannels = 7,
};
enum Status : int64_t { kNalOverflow = 1, kAdtsError = 2, kUnsupportedVideo = 4 };
enum AuFlags : int { kAuKeyframe = 1, kAuSps = 2, kAuPps = 4, kAuAud = 8 };  // au[..][2]

// scratch (int32), element offsets: [tile_cnt: total_tiles | tile_pre: total_tiles | pos: nseg x (max_nal + 1)]
struct IndexScratch { int64_t tile_cnt, tile_pre, pos, end; };
constexpr IndexScratch index_scratch(int64_t total_tiles, int64_t nseg, int64_t max_nal) {
  return {0, total_tiles, 2 * total_tiles, 2 * total_tiles + nseg * (max_nal + 1)};
}
}  // namespace es

// ---------------------------------------------------------------- CRC-32
namespace crc {
constexpr int kGroupBytes = 256;      // data bytes per MFMA output row
constexpr int kTileGroups = 32;       // groups (MFMA rows) per wave tile
constexpr int kTileBytes = kTileGroups * kGroupBytes;
constexpr int kChunkBytes = 4096;     // data bytes per fused decrypt + CRC chunk
constexpr int kNumP = 40;             // P_b tables, b = 0..39  (shift up to 2^39 bytes)
constexpr int kNumQ = 12;             // Q_b tables, b = 0..11  (undo pad < 4096 bytes)
constexpr int kSliceWords = 4 * 256;  // one byte-slice table set (4 KiB)
constexpr int kFusedAesSteps = 8;     // FP4 weight steps of the CRC fused into the decrypt
constexpr int kFusedFoldSteps = 32;   // ... and of the chunk fold
constexpr int kFusedMaskDwords = 64;  // mask dwords per 4096-byte chunk

constexpr int64_t groups(int64_t n) { return (n + kGroupBytes - 1) / kGroupBytes; }
constexpr int64_t tiles(int64_t n) { return (groups(n) + kTileGroups - 1) / kTileGroups; }
// shift tables: P_0..P_39 then Q_0..Q_11, one byte-slice set each
constexpr int64_t kShiftTableWords = int64_t(kNumP + kNumQ) * kSliceWords;
}  // namespace crc
}  // namespace hlsp2p
