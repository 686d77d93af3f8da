// Codec configuration of demuxed and indexed segments for the fMP4 init segment
// (docs/INITSEGMENT.md) — CDNA4 / gfx950.
//
// Input: what ts_demux.hip and es_index.hip leave in HBM.  Output per segment, identical to the
// host implementation runtime/codec.cpp config_segment:
//   ps:    uint8[seg][kPsRows][max_ps]  (the first SPS and PPS NAL units as they are, zero beyond)
//   cinfo: int32[seg][kCinfoWords]      (Cinfo: status, rows, lengths, SPS fields, ADTS fields)
//
// One launch on the caller's stream, one 256-thread workgroup per segment, no scratch:
//   a. row search — rounds of 256 NAL rows, one 16-byte load per lane, a wave ballot for the
//                   types 7 and 8 with a length, the lowest row of each through LDS; the round
//                   loop is workgroup-uniform and ends once both are found.
//   b. byte copy  — wave 0 the SPS, wave 1 the PPS, a lane per 16 stored bytes: five dwords
//                   through the segment's buffer resource (es_dev.h es_segment_rsrc) funnelled to
//                   the NAL's alignment (common.h load16_unaligned), masked to the stored length,
//                   one 16-byte store to ps and, for the SPS, one to LDS.
//   c. unescape   — a lane per SPS byte flags emulation prevention from its two raw
//                   predecessors in LDS; a ballot and popcount prefix with a carry across waves
//                   and rounds compacts the RBSP into a second LDS array.
//   d. parse      — lane 0 runs es::sps_parse on the RBSP while lane 0 of wave 1 takes the ADTS
//                   fields.
//   e. row write  — a lane per cinfo word.
// Steps a, b and c are ps_dev.h, shared with hevc_config.hip.
// No workgroup waits for another one.  The emulation-prevention predicate, sps_parse and the
// ADTS fields are shared/grammar.hpp (namespace es), the same functions runtime/codec.cpp calls.
#include "es_dev.h"
#include "ps_dev.h"

namespace hlsp2p {
namespace dev {

__global__ __launch_bounds__(kPsThreads) void codec_config_kernel(EsBatchView b, int max_ps,
                                                                  uint8_t* __restrict__ ps_all,
                                                                  int32_t* __restrict__ cinfo_all) {
  __shared__ __attribute__((aligned(16))) uint8_t s_raw[es::kMaxPsLimit];   // the SPS as stored
  __shared__ __attribute__((aligned(16))) uint8_t s_rbsp[es::kMaxPsLimit];  // ... and without emulation prevention
  __shared__ int s_found[es::kPsRows];
  __shared__ int s_wave[kPsWaves];
  __shared__ int32_t s_row[es::kCinfoWords];
  const int seg = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const auto c = es_segment(b, seg);
  const es::Segment& sg = c.sg;
  const int cap_es = c.cap;
  const bool avc = sg.info[ts::kVideoType] == ts::kAvc;
  const int R = avc ? static_cast<int>(c.R) : 0;
  if (tid < es::kPsRows) s_found[tid] = kPsNone;
  if (tid < es::kCinfoWords) s_row[tid] = 0;
  __syncthreads();

  // ---- a. the first SPS and PPS rows
  const v4i* rows = reinterpret_cast<const v4i*>(c.ix.nal);  // a table row is 16 bytes of a 16-byte aligned table
  const int types[es::kPsRows] = {7, 8};
  ps_find_rows(rows, R, types, s_found);
  const int found[es::kPsRows] = {s_found[es::kPsSps], s_found[es::kPsPps]};

  // ---- b. both NAL units to ps, the SPS to LDS as well
  int len[es::kPsRows] = {0, 0}, src[es::kPsRows] = {0, 0};
#pragma unroll
  for (int w = 0; w < es::kPsRows; ++w) {
    if (found[w] == kPsNone) continue;
    const v4i row = rows[found[w]];
    src[w] = static_cast<int>(clamp(row[es::kNalOffset], 0, cap_es));
    len[w] = static_cast<int>(clamp(row[es::kNalLength], 0, cap_es - src[w]));
  }
  if (wave < es::kPsRows && lane * 16 < max_ps) {
    const v4u q = ps_copy_lane(es_segment_rsrc(b, seg), src[wave], len[wave], max_ps, lane);
    uint8_t* dst = ps_all + es::ps_bytes(seg, max_ps) + static_cast<int64_t>(wave) * max_ps;
    *reinterpret_cast<v4u*>(dst + lane * 16) = q;
    if (wave == es::kPsSps) *reinterpret_cast<v4u*>(s_raw + lane * 16) = q;
  }
  __syncthreads();

  // ---- c. the SPS without its header byte and emulation prevention
  const bool parse = found[es::kPsSps] != kPsNone && len[es::kPsSps] <= max_ps;  // an overflowed SPS is not parsed
  const int carry = ps_unescape(s_raw, parse ? len[es::kPsSps] : 0, 1, s_rbsp, s_wave);

  // ---- d. one lane parses, one of another wave takes the ADTS fields
  if (tid == 0) {
    int32_t status = 0;
    if (!avc) status |= es::kConfigUnsupportedVideo;
    else status |= (found[es::kPsSps] == kPsNone ? es::kNoSps : 0) | (found[es::kPsPps] == kPsNone ? es::kNoPps : 0);
    if (len[es::kPsSps] > max_ps || len[es::kPsPps] > max_ps) status |= es::kPsOverflow;
    s_row[es::kCSpsNal] = found[es::kPsSps] == kPsNone ? -1 : found[es::kPsSps];
    s_row[es::kCPpsNal] = found[es::kPsPps] == kPsNone ? -1 : found[es::kPsPps];
    s_row[es::kCSpsBytes] = len[es::kPsSps];
    s_row[es::kCPpsBytes] = len[es::kPsPps];
    if (parse) {
      es::SpsFields f;
      const uint8_t* p = s_rbsp;
      if (!es::sps_parse([p](int64_t i) { return p[i]; }, carry, f)) status |= es::kBadSps;
      s_row[es::kCSpsRbspBytes] = carry;
      s_row[es::kCProfileIdc] = f.profile_idc;
      s_row[es::kCProfileCompat] = f.profile_compat;
      s_row[es::kCLevelIdc] = f.level_idc;
      s_row[es::kCChromaFormatIdc] = f.chroma_format_idc;
      s_row[es::kCBitDepthLuma] = f.bit_depth_luma;
      s_row[es::kCBitDepthChroma] = f.bit_depth_chroma;
      s_row[es::kCWidth] = f.width;
      s_row[es::kCHeight] = f.height;
      s_row[es::kCSarWidth] = f.sar_width;
      s_row[es::kCSarHeight] = f.sar_height;
    }
    atomicOr(&s_row[es::kCStatus], status);
  } else if (tid == 64) {
    const es::AudioSpan audio = es::audio_span(sg);
    bool usable = false;
    if (audio.n_adts >= 1 && c.ix.aframes[es::kApesFrames] >= 1) {
      const es::ByteRange r = es::audio_pes_range(es::pes_rows(sg).audio, 0, audio);
      if (r.start + 7 <= r.end) {
        const es::AdtsConfig c = es::adts_config_at(sg.es + audio.off, r.start);
        s_row[es::kCAacObjectType] = c.object_type;
        s_row[es::kCAacRateIndex] = c.rate_index;
        s_row[es::kCAacChannelConfig] = c.channel_config;
        usable = es::adts_config_usable(c);
      }
    }
    if (!usable) atomicOr(&s_row[es::kCStatus], static_cast<int32_t>(es::kNoAudioConfig));
  }
  __syncthreads();

  // ---- e. the row
  if (tid < es::kCinfoWords) cinfo_all[static_cast<int64_t>(seg) * es::kCinfoWords + tid] = s_row[tid];
}

hipError_t launch_codec_config(const CodecConfigArgs& a) {
  const EsBatch& b = a.b;
  if (b.nseg <= 0) return hipSuccess;
  hipLaunchKernelGGL(codec_config_kernel, dim3(b.nseg), dim3(kPsThreads), 0, b.stream, es_batch_view(b),
                     static_cast<int>(a.max_ps), a.ps, a.cinfo);
  return hipGetLastError();
}

}  // namespace dev
}  // namespace hlsp2p
