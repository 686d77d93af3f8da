// Row layouts, status bits, tile geometry and workspace sizes: the only definition of each, for
// the host runtime, the gfx950 kernels and their bindings.  <cstdint> only, constexpr.
#pragma once
#include <cstdint>

namespace hlsp2p {

// elements of a table of `rows` rows of `width` words per segment: a batch's size, and where segment nseg starts
constexpr int64_t table_words(int64_t nseg, int64_t rows, int width) { return nseg * rows * width; }

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

// pes[] (int64): [segment][class][max_pes] rows, -1 rows beyond a class's PES count
constexpr int kPesWords = 3;
enum PesRow : int { kPesEsOffset = 0, kPesPts = 1, kPesDts = 2 };  // offset inside the class's ES
constexpr int64_t pes_words(int64_t nseg, int64_t max_pes) { return nseg * kClasses * max_pes * kPesWords; }

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
enum AuFlags : int { kAuKeyframe = 1, kAuSps = 2, kAuPps = 4, kAuAud = 8 };  // au[..][kAuFlags]

// index tables (int32), -1 rows beyond: nal [segment][max_nal], au and aframes [segment][max_pes]
constexpr int kNalWords = 4;
enum NalRow : int { kNalOffset = 0, kNalLength = 1, kNalType = 2, kNalAu = 3 };  // offset inside the video ES
constexpr int kAuWords = 4;
enum AuRow : int { kAuFirstNal = 0, kAuNalCount = 1, kAuFlags = 2, kAuSize = 3 };
constexpr int kApesWords = 2;  // aframes row: one per audio PES
enum ApesRow : int { kApesFrames = 0, kApesUsed = 1 };  // whole ADTS frames, and their bytes
// One segment's four index tables, or a batch's; I32 / I64 are const where they are only read.
template <class I32, class I64>
struct IndexTables {
  I32 *nal, *au, *aframes;
  I64* sinfo;
};

// scratch (int32), element offsets: [tile_cnt: total_tiles | tile_pre: total_tiles | pos: nseg x (max_nal + 1)]
struct IndexScratch { int64_t tile_cnt, tile_pre, pos, end; };
constexpr IndexScratch index_scratch(int64_t total_tiles, int64_t nseg, int64_t max_nal) {
  return {0, total_tiles, 2 * total_tiles, 2 * total_tiles + nseg * (max_nal + 1)};
}

// ---- remux to fMP4 samples and mdat boxes (docs/REMUX.md)
constexpr int kRinfoWords = 8;
constexpr int64_t kDefaultMaxAframes = 1024;
constexpr int kVsampleWords = 5;  // vsamples row [segment][max_pes], one per access unit
enum VsampleRow : int { kVsOffset = 0, kVsSize = 1, kVsDuration = 2, kVsCts = 3, kVsFlags = 4 };  // offset in the payload
constexpr int kAsampleWords = 2;  // asamples row [segment][max_aframes], one per AAC frame
enum AsampleRow : int { kAsOffset = 0, kAsSize = 1 };
// One segment's three remux tables, or a batch's.
struct RemuxTables {
  int32_t *vsamples, *asamples;
  int64_t* rinfo;
};
constexpr int kRemuxTile = 16384;  // output bytes per workgroup of the copy kernel
constexpr int kOutAlign = 256;     // alignment of a segment's output region on the device
constexpr int32_t kSampleSync = 0x02000000;     // sample_depends_on = 2
constexpr int32_t kSampleNonSync = 0x01010000;  // sample_depends_on = 1, non-sync sample

// rinfo[] row (int64), identical on host and device
enum Rinfo : int {
  kRStatus = 0,
  kVideoPayloadBytes = 1,  // P
  kNumVsamples = 2,
  kAudioBoxOffset = 3,     // A0
  kAudioPayloadBytes = 4,  // Q
  kNumAframes = 5,         // true total, also when the table overflowed
  kVideoBaseDts = 6,       // -1: no sample
  kAudioBasePts = 7,       // -1: no audio PES
};
enum RemuxStatus : int64_t { kTruncated = 1, kAframeOverflow = 2, kBadTimestamps = 4, kRemuxUnsupportedVideo = 8 };

// bytes of a segment's output region: each kept NAL trades a >= 3-byte start code for a 4-byte
// length (P <= video bytes + recorded NALs), video + audio <= cap, two 8-byte box headers and
// at most 15 bytes of padding in front of the audio box
constexpr int64_t remux_out_bytes(int64_t cap, int64_t max_nal) { return cap + max_nal + 32; }
// the video payload may take this much of the region; what is left holds the padding and the audio header
constexpr int64_t remux_video_limit(int64_t cap, int64_t max_nal) { return cap + max_nal; }
// A0, where the audio box starts behind a video payload of P bytes; audio_gap (a multiple of 16,
// default 0) bytes are left free in front of it and make the region that much longer
constexpr int64_t audio_box_offset(int64_t P, int64_t audio_gap) { return (8 + P + audio_gap + 15) & ~int64_t(15); }

// scratch (int32), element offsets inside one segment's slice of `stride` elements:
// [hdr: 8 | vstart: max_nal + 1 | vsrc: max_nal | astart: max_aframes + 1 | asrc: max_aframes]
// hdr = (recorded NALs, recorded frames); *start are payload offsets with the total behind the
// last row, *src the first body byte in the segment's ES
struct RemuxScratch { int64_t vstart, vsrc, astart, asrc, stride, end; };
constexpr RemuxScratch remux_scratch(int64_t nseg, int64_t max_nal, int64_t max_aframes) {
  return {8, 9 + max_nal, 9 + 2 * max_nal, 10 + 2 * max_nal + max_aframes, 10 + 2 * (max_nal + max_aframes),
          nseg * (10 + 2 * (max_nal + max_aframes))};
}

// ---- moof boxes in front of the two mdat boxes (docs/FRAGMENT.md)
// moof{ mfhd, traf{ tfhd, tfdt (v1), trun } } as player/fmp4.py packs it: the video trun has a
// 16-byte entry per sample, the audio tfhd carries two defaults and its trun a 4-byte entry per frame
constexpr int kMoofVideoHead = 88, kMoofVideoEntry = 16;
constexpr int kMoofAudioHead = 96, kMoofAudioEntry = 4;
constexpr int64_t moof_video_bytes(int64_t m) { return kMoofVideoHead + kMoofVideoEntry * m; }
constexpr int64_t moof_audio_bytes(int64_t n) { return kMoofAudioHead + kMoofAudioEntry * n; }
// room in front of a segment's region for the largest video moof: the moof ends where the region starts
constexpr int64_t frag_headroom(int64_t max_pes) {
  return (moof_video_bytes(max_pes) + kOutAlign - 1) / kOutAlign * kOutAlign;
}
// room between the video payload and the audio box for the largest audio moof: the moof ends at A0
constexpr int64_t frag_audio_gap(int64_t max_aframes) { return (moof_audio_bytes(max_aframes) + 15) / 16 * 16; }

// finfo[] row (int64), identical on host and device
constexpr int kFinfoWords = 8;
enum Finfo : int {
  kFStatus = 0,
  kFVideoMoofBytes = 1, kFAudioMoofBytes = 2,
  kFVideoTfdt = 3,  // 90 kHz
  kFAudioTfdt = 4,  // in units of the audio sample rate
  kFTimeBase = 5,   // the base that was used, also when the segment anchored it
  kFNumAsamples = 6,
  kFSpare = 7,      // 0
};
enum FragStatus : int64_t { kTimeClamped = 1, kNoRate = 2 };

// fparams[] row (int64): what the host says about a segment
constexpr int kFparamWords = 8;
enum Fparam : int {
  kFpOutOff = 0,   // where the segment's video mdat starts in out
  kFpRegion = 1,   // bytes of the region from there on: es::remux_out_bytes(cap, max_nal) + audio_gap
  kFpSequence = 2, // mfhd sequence_number, used modulo 2^32
  kFpTimeBase = 3,
  kFpTimeRef = 4,  // -1: none
  kFpAnchor = 5,   // != 0: the segment sets the base from its own first stamp and kFpTimeRef
  kFpSpare0 = 6, kFpSpare1 = 7,
};

// ---- codec configuration for the fMP4 init segment (docs/INITSEGMENT.md)
constexpr int kCinfoWords = 19;
constexpr int64_t kDefaultMaxPs = 256;  // stored bytes per parameter set
constexpr int64_t kMaxPsLimit = 1024;   // max_ps: a positive multiple of kPsAlign up to this
constexpr int kPsAlign = 16;
constexpr bool max_ps_ok(int64_t max_ps) { return max_ps > 0 && max_ps <= kMaxPsLimit && max_ps % kPsAlign == 0; }
constexpr int kPsRows = 2;  // ps [segment][kPsRows][max_ps] (uint8): row 0 the SPS, row 1 the PPS
enum PsRow : int { kPsSps = 0, kPsPps = 1 };
constexpr int64_t ps_bytes(int64_t nseg, int64_t max_ps) { return nseg * kPsRows * max_ps; }

// cinfo[] row (int32), identical on host and device; kCProfileIdc .. kCSarHeight are SpsFields in order
enum Cinfo : int {
  kCStatus = 0,
  kCSpsNal = 1,  // row of the nal table, -1: none
  kCSpsBytes = 2, kCSpsRbspBytes = 3,
  kCPpsNal = 4, kCPpsBytes = 5,
  kCProfileIdc = 6, kCProfileCompat = 7, kCLevelIdc = 8,
  kCChromaFormatIdc = 9, kCBitDepthLuma = 10, kCBitDepthChroma = 11,
  kCWidth = 12, kCHeight = 13, kCSarWidth = 14, kCSarHeight = 15,
  kCAacObjectType = 16, kCAacRateIndex = 17, kCAacChannelConfig = 18,
};
enum ConfigStatus : int32_t {
  kNoSps = 1, kNoPps = 2, kPsOverflow = 4, kBadSps = 8, kConfigUnsupportedVideo = 16, kNoAudioConfig = 32,
};

// ---- HEVC configuration for the hvc1 init segment (docs/INITSEGMENT.md); max_ps as above
constexpr int kHinfoWords = 22;
constexpr int kHpsRows = 3;  // hps [segment][kHpsRows][max_ps] (uint8): the VPS, the SPS, the PPS
enum HpsRow : int { kHpsVps = 0, kHpsSps = 1, kHpsPps = 2 };
constexpr int kHevcVps = 32, kHevcSps = 33, kHevcPps = 34;  // nal_unit_type
constexpr int kHevcNalHeader = 2;                           // header bytes in front of the RBSP
constexpr int64_t hps_bytes(int64_t nseg, int64_t max_ps) { return nseg * kHpsRows * max_ps; }

// hinfo[] row (int32), identical on host and device; kHProfileSpace .. kHHeight are HevcSpsFields in order
enum Hinfo : int {
  kHStatus = 0,
  kHVpsNal = 1,  // row of the nal table, -1: none
  kHVpsBytes = 2,
  kHSpsNal = 3, kHSpsBytes = 4, kHSpsRbspBytes = 5,
  kHPpsNal = 6, kHPpsBytes = 7,
  kHProfileSpace = 8, kHTierFlag = 9, kHProfileIdc = 10, kHProfileCompat = 11,
  kHConstraintHi = 12, kHConstraintLo = 13, kHLevelIdc = 14,
  kHNumTemporalLayers = 15, kHTemporalIdNested = 16,
  kHChromaFormatIdc = 17, kHBitDepthLuma = 18, kHBitDepthChroma = 19, kHWidth = 20, kHHeight = 21,
};
enum HevcStatus : int32_t {
  kHNoVps = 1, kHNoSps = 2, kHNoPps = 4, kHPsOverflow = 8, kHBadSps = 16, kHNotHevc = 32,
};

// ---- HLS SAMPLE-AES decryption of the indexed ES in place (docs/SAMPLEAES.md)
constexpr int kSaWords = 6;
// sainfo[] row (int64), identical on host and device; the counts are integer sums
enum Sainfo : int {
  kSaStatus = 0,
  kSaProtectedNals = 1,
  kSaRemovedBytes = 2,  // emulation-prevention bytes taken out of protected NALs
  kSaVideoBlocks = 3,   // 16-byte cipher blocks
  kSaAudioFrames = 4,   // ADTS frames with at least one cipher block
  kSaAudioBlocks = 5,
};
enum SaStatus : int64_t { kSaTruncated = 1, kSaUnsupportedVideo = 2, kSaUnsupportedAudio = 4, kSaPartialAudio = 8 };
constexpr int kSaRound = 4096;       // raw NAL bytes a workgroup unescapes per round
constexpr int kSaClearLead = 32;     // unescaped bytes in front of a NAL's first cipher block
constexpr int kSaBlockStride = 160;  // one cipher block in ten: 16 encrypted, 144 clear
constexpr int kSaAudioLead = 16;     // clear payload bytes of an ADTS frame behind its header
constexpr int kAesBlock = 16;
constexpr int kAesRoundKeyWords = 44;  // equivalent-inverse-cipher round keys of one AES-128 key

// ---- CEA-608/708 caption data of SEI NAL units (docs/CAPTIONS.md)
constexpr int kCcInfoWords = 8;
constexpr int kCcRowWords = 8;
constexpr int64_t kDefaultMaxCc = 512;
constexpr int64_t kMaxCcLimit = 2048;  // max_cc: 1 .. this
constexpr bool max_cc_ok(int64_t max_cc) { return max_cc >= 1 && max_cc <= kMaxCcLimit; }
constexpr int kCcNalBytes = 1024;   // raw bytes of a candidate NAL that are looked at
constexpr int kCcSlotBytes = 96;    // ccbytes slot: cc_count byte, em_data, at most 31 triples (95 bytes)
constexpr int kCcMaxTriples = 31;   // cc_count is five bits
constexpr int kCcFieldBytes = 64;   // cc608 [segment][max_cc][2][kCcFieldBytes]: at most 31 pairs of two bytes per field
constexpr int kCcHeadBytes = 8;     // of a matched message: country, provider (2), 'GA94', type code; the sample starts behind
constexpr int kSeiH264 = 6, kSeiHevcPrefix = 39;  // nal_unit_type of a candidate
constexpr int kSeiUserDataT35 = 4;                // payloadType user_data_registered_itu_t_t35

// ccsamples[] row (int32) [segment][max_cc], -1 rows beyond the recorded samples
enum CcRow : int {
  kCrNal = 0, kCrAu = 1,
  kCrSize = 2,   // 2 + 3 cc_count
  kCrCount = 3,  // cc_count
  kCrOrder = 4,  // presentation rank among the recorded samples
  kCrField1Pairs = 5, kCrField2Pairs = 6,
  kCrFlags = 7,  // CcFlags
};
enum CcFlags : int { kCcProcess = 1 };  // process_cc_data_flag, bytes[0] & 0x40

// ccinfo[] row (int64), identical on host and device; the counts are integer sums
enum Ccinfo : int {
  kCiStatus = 0,
  kCiNumSei = 1,      // candidates walked
  kCiNumSamples = 2,  // true total, also when the table overflowed
  kCiNumTriples = 3,  // of the recorded samples, as the two pair counts
  kCiField1Pairs = 4, kCiField2Pairs = 5,
  kCiFirstPts = 6, kCiLastPts = 7,  // min / max over the recorded samples, -1 without one
};
enum CcStatus : int64_t { kCcTruncated = 1, kCcUnsupportedVideo = 2, kCcOverflow = 4, kCcSeiClipped = 8 };
// One segment's five caption tables, or a batch's.
struct CcTables {
  int32_t* samples;  // [max_cc][kCcRowWords]
  int64_t* pts;      // [max_cc]
  uint8_t* bytes;    // [max_cc][kCcSlotBytes]
  uint8_t* cc608;    // [max_cc][2][kCcFieldBytes]
  int64_t* info;     // [kCcInfoWords]
};

// scratch (int32) between the two caption kernels, element offsets:
// [flag: nseg x max_nal | hit: nseg x max_nal x kCcSlotBytes / 4], hit 16-byte aligned.
// flag of row k < R = CcScratchFlag bits | size << 8; hit holds the slot of a row whose flag has kCfHit
enum CcScratchFlag : int { kCfCandidate = 1, kCfClipped = 2, kCfHit = 4 };
constexpr int kCfSizeShift = 8;
struct CcScratch { int64_t flag, hit, end; };
constexpr CcScratch cc_scratch(int64_t nseg, int64_t max_nal) {
  return {0, (nseg * max_nal + 3) / 4 * 4, (nseg * max_nal + 3) / 4 * 4 + nseg * max_nal * (kCcSlotBytes / 4)};
}

// ---- packed audio: ID3v2 tags in front of raw ADTS frames (docs/PACKEDAUDIO.md).  info / pes have
// the layouts of ts:: above, nal / au / aframes / sinfo those of the index; nal has one row.
constexpr int kPackedFramesPerPes = 4;  // G: ADTS frames per audio PES row
constexpr int kPackedMaxTags = 8;       // leading tags that are looked at
constexpr int kPackedMaxId3Frames = 32; // frames read inside one tag
constexpr int kPackedNalRows = 1;       // max_nal of the views: there is no video
constexpr int kPackedTile = 32768;      // bytes of a segment staged in LDS per round of the frame walk
constexpr int64_t kPackedMaxPesLimit = 4096;  // max_pes: 1 .. this (the walk keeps max_pes + 1 offsets in LDS)
constexpr bool packed_max_pes_ok(int64_t v) { return v >= 1 && v <= kPackedMaxPesLimit; }
constexpr int kAacFrameSamples = 1024;
constexpr int kPainfoWords = 8;
// painfo[] row (int64), identical on host and device
enum Painfo : int {
  kPaStatus = 0,
  kPaId3Bytes = 1,    // T: where the audio starts
  kPaNumTags = 2,     // whole leading tags
  kPaTimestamp = 3,   // 33 bits, -1: none
  kPaNumFrames = 4,   // true total
  kPaStopOffset = 5,  // where the frame walk ended
  kPaSampleRate = 6, kPaChannels = 7,
};
enum PackedStatus : int64_t {
  kPaNoTimestamp = 1, kPaBadId3 = 2, kPaNoFrame = 4, kPaTrailingBytes = 8, kPaPesOverflow = 16, kPaBadRate = 32,
};
// the bits that make a segment unusable for a player
constexpr int64_t kPaFatalMask = kPaNoTimestamp | kPaBadId3 | kPaNoFrame | kPaBadRate;
// One segment's seven output tables, or a batch's.
struct PackedTables {
  int64_t *info, *pes;
  IndexTables<int32_t, int64_t> ix;
  int64_t* painfo;
};

// ---- MPEG audio (MPEG-1/2/2.5 Layer I-III) tracks of TS segments, behind the remux (docs/MPEGAUDIO.md)
constexpr int kMpainfoWords = 8;
// mpainfo[] row (int64), identical on host and device; with kMpaNotMpegAudio or kMpaNoAudioConfig every other slot is 0
enum Mpainfo : int {
  kMpStatus = 0,
  kMpNumFrames = 1,  // true total, also when the table overflowed
  kMpSampleRate = 2, kMpChannels = 3,
  kMpVersion = 4,    // 1, 2 or 25
  kMpLayer = 5,      // 1, 2 or 3
  kMpFrameSamples = 6,
  kMpBitrate = 7,    // of the first frame, bit/s
};
enum MpaStatus : int64_t {
  kMpaNotMpegAudio = 1, kMpaNoAudioConfig = 2, kMpaError = 4, kMpaFormatChange = 8, kMpaAframeOverflow = 16,
};
// mframes[] row (int32) [segment][max_pes]: ApesRow (whole frames, and their bytes), -1 rows beyond the audio PES
// One segment's outputs, or a batch's: two tables of its own, and the remux's asamples and rinfo.
struct MpaTables {
  int32_t* mframes;
  int64_t* mpainfo;
  int32_t* asamples;
  int64_t* rinfo;
};
// scratch (int32), element offsets inside one segment's slice of `stride` elements:
// [hdr: 8 | pstart: max_pes + 1 | psrc: max_pes]
// hdr = (walked PES); pstart are the payload offsets of each PES's first frame with the total
// behind the last row, psrc the PES's first byte in the segment's ES
struct MpaScratch { int64_t pstart, psrc, stride, end; };
constexpr MpaScratch mpa_scratch(int64_t nseg, int64_t max_pes) {
  return {8, 9 + max_pes, 9 + 2 * max_pes, nseg * (9 + 2 * max_pes)};
}
// ---- AC-3 / E-AC-3 tracks of TS segments, behind the remux (docs/AC3AUDIO.md).  The scratch is es::mpa_scratch.
constexpr int kAc3FrameSamples = 1536;
constexpr int kAc3KindAc3 = 1, kAc3KindEac3 = 2;
constexpr int32_t kAc3NoKey = -1;  // the key of a header whose layout is unsupported: equal to no frame's key
constexpr int kAc3infoWords = 16;
// ac3info[] row (int64), identical on host and device; with kAc3NotDolbyAudio or kAc3NoAudioConfig every other slot is 0
enum Ac3info : int {
  kAcStatus = 0,
  kAcNumFrames = 1,  // true total, also when the table overflowed
  kAcSampleRate = 2, kAcChannels = 3,
  kAcKind = 4,       // kAc3KindAc3 / kAc3KindEac3
  kAcBsid = 5,
  kAcFrameSamples = 6,
  kAcBitrate = 7,    // of the first frame, bit/s
  kAcFscod = 8, kAcBsmod = 9, kAcAcmod = 10, kAcLfeon = 11,
  kAcBitRateCode = 12,  // AC-3: frmsizecod >> 1 (dac3)
  kAcDataRate = 13,     // E-AC-3: kbit/s (dec3)
  kAcFirstFrameBytes = 14,
  kAcSpare = 15,
};
enum Ac3Status : int64_t {
  kAc3NotDolbyAudio = 1, kAc3NoAudioConfig = 2, kAc3Error = 4, kAc3FormatChange = 8, kAc3AframeOverflow = 16,
  kAc3UnsupportedLayout = 32,
};
// dframes[] row (int32) [segment][max_pes]: ApesRow, as mframes
// One segment's outputs, or a batch's: three tables of its own, and the remux's asamples and rinfo.
struct Ac3Tables {
  int32_t* dframes;
  int64_t* ac3info;
  int64_t* mpainfo;       // a row in Mpainfo's layout for fragment_moof
  const int64_t* mpa_in;  // the MPEG audio op's mpainfo (copied for the segments of other codecs), or null
  int32_t* asamples;
  int64_t* rinfo;
};
}  // namespace es

// ---------------------------------------------------------------- fragmented MP4 demux (docs/FMP4DEMUX.md)
namespace mp4 {
constexpr int kTracks = 2;  // slot 0 the video track, slot 1 the audio track
constexpr int64_t kDefaultMaxMoof = 64, kDefaultMaxRun = 128, kDefaultMaxEmsg = 16;
constexpr int64_t kMaxBoxRows = 256;  // max_moof, max_run, max_emsg: 1 .. this (a lane per row in one workgroup)
constexpr bool max_rows_ok(int64_t v) { return v >= 1 && v <= kMaxBoxRows; }

// tracks[] row (int64) [segment][kTracks]: what the init segment says about a track
constexpr int kTrackWords = 8;
enum TrackRow : int {
  kTkId = 0,             // track_ID, <= 0: the slot is empty
  kTkKind = 1,           // TrackKind
  kTkCodecType = 2,      // slot 0: 0x1B / 0x24 / 0 (no NAL index); slot 1: 0x0F for mp4a, else 0
  kTkNalLengthSize = 3,  // 1, 2 or 4 where kTkCodecType is a video type
  kTkDefDuration = 4, kTkDefSize = 5, kTkDefFlags = 6,  // the trex defaults
  kTkSpare = 7,
};
enum TrackKind : int { kKindNone = 0, kKindVideo = 1, kKindAudio = 2 };

// minfo[] row (int64); the per-track family is kMTrack0 + kMTrackWords * slot + MinfoTrack
constexpr int kMTrack0 = 6, kMTrackWords = 6;
constexpr int kMinfoWords = kMTrack0 + kTracks * kMTrackWords;
enum Minfo : int {
  kMStatus = 0,
  kMNumMoof = 1,       // true total
  kMFirstSequence = 2, // mfhd sequence_number of the first moof, -1: none
  kMNumRun = 3,        // true total of the configured tracks' trun boxes
  kMNumOtherTraf = 4,
  kMNumEmsg = 5,       // true total
};
enum MinfoTrack : int {
  kMtNumSamples = 0,  // true total
  kMtBaseTime = 1,    // decode time of the track's first sample-bearing traf, -1: none
  kMtDuration = 2,    // over all samples
  kMtMinPts = 3, kMtMaxPts = 4,  // over the recorded samples, -1 without one
  kMtFirstSync = 5,   // among the recorded samples, -1: none
};
enum Status : int64_t {
  kBadBox = 1, kMoofOverflow = 2, kEmsgOverflow = 4, kRunOverflow = 8, kNoTfdt = 16, kSampleOutOfRange = 32,
  kSampleOverflow = 64, kNalError = 128, kBadTimestamps = 256,
};

// msamples[] row (int32) [segment][kTracks][max_pes], -1 rows beyond the recorded samples
constexpr int kMsampleWords = 4;
enum MsampleRow : int { kMsSize = 0, kMsDuration = 1, kMsCts = 2, kMsFlags = 3 };
constexpr uint32_t kSampleNonSyncBit = 0x00010000;  // sample_is_non_sync_sample

// runs[] row (int64) [segment][max_run], -1 rows beyond the recorded runs; the sample pass reads it
constexpr int kRunWords = 16;
enum RunRow : int {
  kRnTrack = 0, kRnMoof = 1,
  kRnFirst = 2,    // the run's first sample among its track's samples
  kRnCount = 3,    // whole entries that fit the box
  kRnEntries = 4,  // offset of the first entry in the segment
  kRnFlags = 5,    // tr_flags | version << 24
  kRnTrafRun = 6,  // 0: the first run of its traf
  kRnDefDuration = 7, kRnDefSize = 8, kRnDefFlags = 9,  // tfhd, else trex
  kRnFirstFlags = 10,                                   // first_sample_flags, -1: absent
  kRnStart = 11, kRnStartSample = 12,  // sample s of the run starts at kRnStart + sizes of [kRnStartSample, s)
  kRnTime = 13, kRnTimeSample = 14,    // ... and is decoded at kRnTime + durations of [kRnTimeSample, s)
  kRnSpare = 15,
};

// emsg[] row (int64) [segment][max_emsg], one per top-level emsg box, a dropped or unrecorded row all -1
constexpr int kEmsgWords = 12;
enum EmsgRow : int {
  kEmOffset = 0, kEmSize = 1, kEmVersion = 2, kEmTimescale = 3,
  kEmTime = 4,         // presentation_time (v1) or presentation_time_delta (v0)
  kEmTimeIsDelta = 5,
  kEmDuration = 6, kEmId = 7,
  kEmDataOffset = 8, kEmDataLength = 9,
  kEmIsId3 = 10, kEmSpare = 11,
};

// One segment's output tables, or a batch's.  info / pes / nal / au / aframes / sinfo have the
// layouts of ts:: and es:: above.
struct Tables {
  int64_t* minfo;     // [kMinfoWords]
  int32_t* msamples;  // [kTracks][max_pes][kMsampleWords]
  int64_t* runs;      // [max_run][kRunWords]
  int64_t* emsg;      // [max_emsg][kEmsgWords]
  int64_t *info, *pes;
  es::IndexTables<int32_t, int64_t> ix;
};
struct Limits { int64_t max_pes, max_nal, max_moof, max_run, max_emsg; };

// ---- cbcs decryption of a demuxed batch (docs/CBCS.md)
// protection[] row (int64) [segment][kTracks]: what the init segment's tenc says about a track
constexpr int kProtWords = 8;
enum ProtRow : int {
  kPrProtected = 0,    // 1: the track's samples are looked at
  kPrCrypt = 1, kPrSkip = 2,  // the pattern in 16-byte blocks; skip 0: every block
  kPrIvSize = 3,       // Per_Sample_IV_Size: 0, 8 or 16
  kPrConstIvSize = 4,  // 0, 8 or 16; used when kPrIvSize is 0
};
// cinfo[] row (int64); every count is an integer sum
constexpr int kCbInfoWords = 8;
enum CbInfo : int {
  kCbStatus = 0,
  kCbNumRanges = 1,  // true total of the ranges with a cipher block
  kCbVideoSamples = 2, kCbAudioSamples = 3,  // samples with a cipher block
  kCbVideoBlocks = 4, kCbAudioBlocks = 5,    // cipher blocks, the unrecorded ranges' included
  kCbNumSenc = 6,    // senc boxes that were read
  kCbSpare = 7,
};
enum CbStatus : int64_t { kCbRangeOverflow = 1, kCbNoSenc = 2, kCbBadSenc = 4, kCbDemuxDamaged = 8, kCbOverlap = 16 };
// the minfo status bits that make a demux "damaged" for the decrypt
constexpr int64_t kCbDamagedMask =
    kBadBox | kMoofOverflow | kEmsgOverflow | kRunOverflow | kSampleOverflow | kSampleOutOfRange;
// ranges[] row (int32) [segment][max_range], -1 rows beyond the recorded ranges
constexpr int kRangeWords = 4;
enum RangeRow : int {
  kRgOffset = 0, kRgLength = 1,
  kRgSample = 2,  // track slot << kRgTrackShift | sample
  kRgRank = 3,    // the range's first cipher block among the segment's
};
constexpr int kRgTrackShift = 30;
constexpr int64_t kMaxRangeLimit = 65536, kDefaultMaxRange = 4096;
constexpr bool max_range_ok(int64_t v) { return v >= 1 && v <= kMaxRangeLimit; }
// scratch row (int32) [segment][kTracks][max_pes]: a recorded sample's auxiliary data
constexpr int kAuxWords = 4;
enum AuxRow : int {
  kAxEntry = 0,  // offset of its senc entry in the segment, -1: none
  kAxSubs = 1,   // subsample_count, -1: the entry has no subsample table
  kAxRun = 2,    // its row of runs
  kAxSpare = 3,
};
constexpr int64_t cbcs_scratch(int64_t nseg, int64_t max_pes) { return nseg * kTracks * max_pes * kAuxWords; }
constexpr int kCbTileBlocks = 256;  // cipher blocks per tile of the decrypt, a lane each

// ---- cenc (AES-CTR) decryption of a demuxed batch (docs/CENC.md).  The protection row, the
// status bits, the scratch row, kRgTrackShift and the max_range limits are the cbcs ones above.
// cinfo[] row (int64)
constexpr int kCnInfoWords = 8;
enum CnInfo : int {
  kCnStatus = 0,
  kCnNumRanges = 1,  // true total of the ranges of at least one byte
  kCnVideoSamples = 2, kCnAudioSamples = 3,  // samples with a protected byte
  kCnVideoBytes = 4, kCnAudioBytes = 5,      // protected bytes, the unrecorded ranges' included
  kCnNumSenc = 6,    // senc boxes that were read
  kCnNumUnits = 7,   // keystream units, the unrecorded ranges' included
};
// ranges[] row (int32) [segment][max_range], -1 rows beyond the recorded ranges
constexpr int kCnRangeWords = 8;
enum CnRangeRow : int {
  kCnOffset = 0, kCnLength = 1,
  kCnSample = 2,     // track slot << kRgTrackShift | sample
  kCnRank = 3,       // the range's first unit among the segment's
  kCnStreamPos = 4,  // protected bytes of the sample in front of the range
  kCnIvOffset = 5,   // where the sample's senc IV stands in the segment, -1: a constant or the job's IV
  kCnSpare0 = 6, kCnSpare1 = 7,  // 0
};
// units per tile of the decrypt: 1024 lanes x kCnLaneUnits
constexpr int kCnLaneUnits = 4;
constexpr int kCnTileUnits = 1024 * kCnLaneUnits;
// host bound of one segment's units: a range of len bytes has at most len / 16 + 2 (a keystream
// block cut at both ends), and the recorded ranges share no byte
constexpr int64_t cenc_unit_bound(int64_t cap, int64_t max_range) { return cap / 16 + 2 * max_range; }
}  // namespace mp4

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
