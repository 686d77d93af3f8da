// Host side of every kernel launch: one argument struct and one declaration per launcher, included
// by the defining .hip file and by every caller.  Device pointers; optional groups default to off.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstdint>

#include "layout.hpp"

namespace hlsp2p {
namespace dev {

// Packet-header records: the decrypt writes ts::header_records(n) per segment, the demux scan reads them.
struct HeaderRecords {
  const int64_t* off = nullptr;  // [nseg] the segment's first record
  void* rec = nullptr;
};

// What a CRC combine writes: crc_out[nseg], ok_out = (expect == crc), scatter_out[scatter_idx] = crc.
struct CrcResults {
  uint32_t* crc_out;
  const uint32_t* expect = nullptr;
  uint8_t* ok_out = nullptr;
  const int64_t* scatter_idx = nullptr;
  uint32_t* scatter_out = nullptr;
  int64_t scatter_n = 0;
};

struct AesDecryptArgs {
  const uint8_t* src;
  uint8_t* dst;
  const int64_t *src_off, *dst_off, *blk_prefix, *chunk_prefix;
  const uint32_t *drk, *iv, *td0;
  const uint8_t* isb;
  int64_t* out_len;
  int nseg;
  int64_t total_chunks;
  int num_cu;
  hipStream_t stream;
  struct FusedCrc {  // CRC-32 of the ciphertext; mask_off == nullptr: off
    const int64_t* mask_off = nullptr;
    const void* wfrag = nullptr;
    uint32_t* masks = nullptr;
  } crc;
  HeaderRecords hdr;
};
int aes_chunk_blocks();
hipError_t launch_aes128_cbc_decrypt(const AesDecryptArgs& a);

struct Crc32BatchArgs {
  const uint8_t* buf;
  const int64_t *seg_off, *seg_len, *tile_prefix, *res_off;
  const void* wfrag;
  bool fp4;
  const uint32_t* tables;  // [crc::kShiftTableWords]
  uint32_t* residues;
  CrcResults out;
  const int64_t* keys = nullptr;  // [nseg][4]: expect / scatter values are bound to the key
  int nseg;
  int64_t total_tiles;
  int num_cu;
  hipStream_t stream;
};
hipError_t launch_crc32_batch(const Crc32BatchArgs& a);

struct Crc32FromMasksArgs {  // second level of the CRC fused into the decrypt
  const uint32_t* masks;
  const void* wfold;
  const int64_t *chunk_off, *seg_len;
  const uint32_t* tables;  // [crc::kShiftTableWords]
  uint32_t* chunk_res;
  CrcResults out;
  int nseg;
  hipStream_t stream;
};
hipError_t launch_crc32_from_masks(const Crc32FromMasksArgs& a);

struct TsDemuxArgs {
  const uint8_t* buf;
  const int64_t *seg_off, *seg_len, *blk_prefix;
  int nseg;
  int64_t total_blocks;
  uint32_t* meta;  // meta, pts_dts, aux: ts::demux_workspace(total_blocks, nseg)
  int64_t* pts_dts;
  int32_t* aux;
  uint8_t* es;
  const int64_t* es_off;
  int64_t* pes;
  int64_t max_pes;
  int64_t* info;
  hipStream_t stream;
  HeaderRecords hdr;
};
hipError_t launch_ts_demux(const TsDemuxArgs& a);

// A demuxed batch as the index, the remux and the codec configuration take it: launch_ts_demux's
// outputs, the host caps and a tile space over them (none for an op of one workgroup per
// segment), and the batch's four index tables.
struct EsBatch {
  const uint8_t* es;
  int64_t es_numel;
  const int64_t *es_off, *cap, *tile_prefix;
  int nseg;
  int64_t total_tiles;
  const int64_t *info, *pes;
  int64_t max_pes, max_nal;
  es::IndexTables<int32_t, int64_t> ix;
  hipStream_t stream;
};

struct EsIndexArgs {
  EsBatch b;         // tiles of cap; ix is written
  int32_t* scratch;  // es::index_scratch(total_tiles, nseg, max_nal)
};
int es_index_tile_bytes();
hipError_t launch_es_index(const EsIndexArgs& a);

struct RemuxArgs {
  EsBatch b;  // tiles of es::remux_out_bytes(cap, max_nal) + audio_gap; ix is launch_es_index's output, only read
  int64_t max_aframes;
  int32_t* scratch;  // es::remux_scratch(nseg, max_nal, max_aframes)
  es::RemuxTables t;
  uint8_t* out;
  const int64_t* out_off;
  int64_t audio_gap = 0;  // free bytes in front of the audio box, a non-negative multiple of 16
};
int remux_tile_bytes();
hipError_t launch_remux(const RemuxArgs& a);

// mpeg_audio.hip: the MPEG audio frames of every segment of a remuxed batch (docs/MPEGAUDIO.md),
// behind launch_remux on the same out, asamples and rinfo.
struct MpegAudioArgs {
  EsBatch b;              // tiles of `region`; ix is not used (all null), max_nal 0
  const int64_t* region;  // [nseg] bytes of each output region, the audio gap included: what launch_remux was given
  int64_t max_aframes;
  int32_t* scratch;  // es::mpa_scratch(nseg, max_pes)
  es::MpaTables t;   // asamples and rinfo are launch_remux's
  uint8_t* out;
  const int64_t* out_off;
};
int mpeg_audio_tile_bytes();
hipError_t launch_mpeg_audio(const MpegAudioArgs& a);

// ac3_audio.hip: the AC-3 / E-AC-3 syncframes of every segment of a remuxed batch (docs/AC3AUDIO.md),
// behind launch_remux (and launch_mpeg_audio) on the same out, asamples and rinfo.
struct Ac3AudioArgs {
  EsBatch b;              // tiles of `region`; ix is not used (all null), max_nal 0
  const int64_t* region;  // [nseg] bytes of each output region, the audio gap included: what launch_remux was given
  int64_t max_aframes;
  int32_t* scratch;  // es::mpa_scratch(nseg, max_pes), not launch_mpeg_audio's
  es::Ac3Tables t;   // asamples and rinfo are launch_remux's; mpa_in launch_mpeg_audio's mpainfo or null
  uint8_t* out;
  const int64_t* out_off;
};
int ac3_audio_tile_bytes();
hipError_t launch_ac3_audio(const Ac3AudioArgs& a);

// fragment.hip: the two moof boxes of every segment of a remuxed batch (docs/FRAGMENT.md), written
// into the room launch_remux's caller left: headroom bytes in front of each region, audio_gap in
// front of each audio box.  One workgroup per segment; a segment whose fparams row does not lie
// inside out (16-byte aligned, headroom in front, region behind) is left alone, finfo row included.
struct FragmentArgs {
  const int64_t* rinfo;     // launch_remux's three tables, only read
  const int32_t* vsamples;  // nseg x max_pes x es::kVsampleWords
  const int32_t* asamples;  // nseg x max_aframes x es::kAsampleWords
  const int64_t* sinfo;     // launch_es_index's: the audio sample rate
  const int64_t* fparams;   // nseg x es::kFparamWords
  int64_t max_pes, max_aframes;
  int64_t headroom;   // >= es::frag_headroom(max_pes)
  int64_t audio_gap;  // >= es::frag_audio_gap(max_aframes), a multiple of 16: what launch_remux took
  uint8_t* out;       // 16-byte aligned
  int64_t out_numel;
  int64_t* finfo;  // nseg x es::kFinfoWords
  const int64_t* mpainfo = nullptr;  // nseg x es::kMpainfoWords, launch_mpeg_audio's: frame and rate of an MPEG audio track
  int nseg;
  hipStream_t stream;
};
hipError_t launch_fragment_moof(const FragmentArgs& a);

struct CodecConfigArgs {
  EsBatch b;       // no tile space (tile_prefix == nullptr, total_tiles == 0); ix is only read
  int64_t max_ps;  // es::max_ps_ok(max_ps)
  uint8_t* ps;     // es::ps_bytes(nseg, max_ps)
  int32_t* cinfo;  // nseg x es::kCinfoWords
};
hipError_t launch_codec_config(const CodecConfigArgs& a);

struct HevcConfigArgs {
  EsBatch b;       // as CodecConfigArgs
  int64_t max_ps;  // es::max_ps_ok(max_ps)
  uint8_t* hps;    // es::hps_bytes(nseg, max_ps)
  int32_t* hinfo;  // nseg x es::kHinfoWords
};
hipError_t launch_hevc_config(const HevcConfigArgs& a);

struct SampleAesArgs {
  EsBatch b;                   // no tile space: the grid is max_pes x nseg x 2 (access units, audio PES)
  uint8_t* es;                 // b.es, rewritten in place; b.ix.nal's length column is rewritten too
  const uint32_t* round_keys;  // nseg x es::kAesRoundKeyWords, little-endian words of the equivalent inverse cipher
  const uint8_t* iv;           // nseg x es::kAesBlock, 16-byte aligned
  const uint8_t* enable;       // nseg; 0: the segment is left alone, its sainfo row is zero
  const uint32_t* td;          // 256 words: TdL
  const uint8_t* isb;          // 256 bytes: the inverse S-box
  int64_t* sainfo;             // nseg x es::kSaWords
};
int sample_aes_round_bytes();
hipError_t launch_sample_aes(const SampleAesArgs& a);

struct CcExtractArgs {
  EsBatch b;              // no tile space: cc_scan_kernel's grid is ceil(max_nal / 64) x nseg, cc_pack_kernel's nseg; ix is only read
  const uint8_t* enable;  // nseg; 0: the segment gets the fill values and an all-zero ccinfo row
  int64_t max_cc;         // es::max_cc_ok(max_cc)
  int32_t* scratch;       // es::cc_scratch(nseg, max_nal), 16-byte aligned
  es::CcTables t;         // 16-byte aligned each
};
hipError_t launch_cc_extract(const CcExtractArgs& a);

struct Mp4DemuxArgs {
  const uint8_t* buf;  // segment i is buf[off[i], off[i] + clamp(len[i], 0, cap[i])), only read; off 16-byte aligned
  int64_t buf_numel;
  const int64_t *off, *len, *cap;
  const int64_t* tracks;  // nseg x mp4::kTracks x mp4::kTrackWords
  int nseg;
  mp4::Limits lim;  // max_pes, max_nal positive; max_moof, max_run, max_emsg mp4::max_rows_ok
  mp4::Tables t;    // every table 16-byte aligned; runs is also the scratch between the first two kernels
  hipStream_t stream;
};
hipError_t launch_mp4_demux(const Mp4DemuxArgs& a);

// packed_audio.hip: ID3v2 tags in front of raw ADTS frames (docs/PACKEDAUDIO.md).  One workgroup per
// segment; info / pes as launch_ts_demux writes them, t.ix as launch_es_index does with one nal row.
struct PackedAudioArgs {
  const uint8_t* buf;  // segment i is buf[off[i], off[i] + clamp(len[i], 0, cap[i])), only read; off 16-byte aligned
  int64_t buf_numel;
  const int64_t *off, *len, *cap;
  int nseg;
  int64_t max_pes;     // es::packed_max_pes_ok
  es::PackedTables t;  // au, aframes and nal 16-byte aligned
  bool staged = true;  // false: the frame chain is walked in global memory (the variant that was measured against)
  hipStream_t stream;
};
int packed_audio_tile_bytes();
hipError_t launch_packed_audio(const PackedAudioArgs& a);

struct CbcsArgs {
  const uint8_t* src;  // the demuxed segments, only read: segment i is src[src_off[i], + clamp(info[i].video_bytes, 0, cap[i]))
  int64_t src_numel;
  const int64_t *src_off, *cap;
  uint8_t* dst;            // 16-byte aligned; holds a copy of every enabled segment at dst_off[i] (16-byte aligned)
  const int64_t* dst_off;
  const int64_t *info, *pes, *minfo, *runs;  // launch_mp4_demux's outputs, only read
  const int32_t* msamples;
  int64_t max_pes, max_run;
  const int64_t* prot;         // nseg x mp4::kTracks x mp4::kProtWords
  const uint8_t* const_iv;     // nseg x mp4::kTracks x 16, 16-byte aligned, padded with zeros
  const uint8_t* iv;           // nseg x 16, 16-byte aligned: for a track without an IV of its own
  const uint32_t* round_keys;  // nseg x es::kAesRoundKeyWords, as SampleAesArgs
  const uint8_t* enable;       // nseg; 0: the segment is left alone, its cinfo row is zero
  const uint32_t* td;
  const uint8_t* isb;
  int64_t max_range;   // mp4::max_range_ok
  int64_t max_blocks;  // host bound of one segment's cipher blocks: max(cap) / 16
  int32_t* scratch;    // mp4::cbcs_scratch(nseg, max_pes), 16-byte aligned
  int32_t* ranges;     // nseg x max_range x mp4::kRangeWords, 16-byte aligned
  int64_t* cinfo;      // nseg x mp4::kCbInfoWords
  int nseg;
  hipStream_t stream;
};
hipError_t launch_cbcs(const CbcsArgs& a);

// cenc.hip: the arguments of launch_cbcs with, in t, round_keys the forward ones (little-endian
// words), td the forward table TeL, isb the S-box, ranges rows of mp4::kCnRangeWords, cinfo rows of
// mp4::kCnInfoWords, and max_blocks unused
struct CencArgs {
  CbcsArgs t;
  int64_t max_cap;  // host bound of one segment's bytes: max(cap)
  int num_cu;       // workgroups of the persistent units kernel
};
hipError_t launch_cenc(const CencArgs& a);

struct SegmentCopyArgs {
  const uint8_t* src;
  uint8_t* dst;
  const int64_t *src_off, *dst_off, *len, *chunk_prefix;
  int ncopy;
  int64_t total_chunks;
  hipStream_t stream;
};
hipError_t launch_segment_copy(const SegmentCopyArgs& a);

}  // namespace dev
}  // namespace hlsp2p
