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
//                   through the segment's buffer resource funnelled to the NAL's alignment
//                   (v_alignbyte), masked to the stored length, one 16-byte store to ps and, for
//                   the SPS, one to LDS.
//   c. unescape   — a lane per SPS byte flags emulation prevention from its two raw
//                   predecessors in LDS; a ballot and popcount prefix with a carry across waves
//                   and rounds compacts the RBSP into a second LDS array.
//   d. parse      — lane 0 runs es::sps_parse on the RBSP while lane 0 of wave 1 takes the ADTS
//                   fields.
//   e. row write  — a lane per cinfo word.
// No workgroup waits for another one.  The emulation-prevention predicate, sps_parse and the
// ADTS fields are shared/grammar.hpp (namespace es), the same functions runtime/codec.cpp calls.
#include "common.h"
#include "grammar.hpp"
#include "launch.h"

namespace hlsp2p {
namespace dev {

constexpr int kCcThreads = 256;
constexpr int kCcWaves = kCcThreads / 64;
constexpr int kCcNone = 0x7fffffff;
static_assert(es::kMaxPsLimit / es::kPsAlign <= 64, "a wave copies a parameter set, a lane per 16 bytes");
static_assert(es::kPsAlign == 16 && es::kNalWords == 4, "16-byte stores, 16-byte NAL rows");

__global__ __launch_bounds__(kCcThreads) void codec_config_kernel(
    const uint8_t* __restrict__ es, int64_t es_numel, const int64_t* __restrict__ es_off,
    const int64_t* __restrict__ cap, const int64_t* __restrict__ info, const int64_t* __restrict__ pes,
    int64_t max_pes, int64_t max_nal, const int32_t* __restrict__ nal_all, const int32_t* __restrict__ au_all,
    const int32_t* __restrict__ af_all, const int64_t* __restrict__ sinfo, int max_ps, uint8_t* __restrict__ ps_all,
    int32_t* __restrict__ cinfo_all) {
  typedef unsigned int v4u __attribute__((ext_vector_type(4)));
  typedef int v4i __attribute__((ext_vector_type(4)));
  __shared__ __attribute__((aligned(16))) uint8_t s_raw[es::kMaxPsLimit];   // the SPS as stored
  __shared__ __attribute__((aligned(16))) uint8_t s_rbsp[es::kMaxPsLimit];  // ... and without emulation prevention
  __shared__ int s_found[es::kPsRows];
  __shared__ int s_wave[kCcWaves];
  __shared__ int32_t s_row[es::kCinfoWords];
  const int seg = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  es::Segment sg = es::segment_at(es, es_off, cap, info, pes, max_pes, max_nal, seg);
  sg.cap = clamp(sg.cap, 0, 0x7fffffff);
  const es::IndexTables<const int32_t, const int64_t> ix =
      es::index_tables_at<const int32_t, const int64_t>({nal_all, au_all, af_all, sinfo}, sg, seg);
  const int cap_es = static_cast<int>(sg.cap);
  const bool avc = sg.info[ts::kVideoType] == ts::kAvc;
  const int R = avc ? static_cast<int>(es::video_rows(es::video_span(sg), ix.sinfo[es::kNumNal], max_nal)) : 0;
  if (tid < es::kPsRows) s_found[tid] = kCcNone;
  if (tid < es::kCinfoWords) s_row[tid] = 0;
  __syncthreads();

  // ---- a. the first SPS and PPS rows
  const v4i* rows = reinterpret_cast<const v4i*>(ix.nal);  // a table row is 16 bytes of a 16-byte aligned table
  for (int kb = 0; kb < R; kb += kCcThreads) {  // R is workgroup-uniform
    const int k = kb + tid;
    int type = -1;
    if (k < R) {
      const v4i row = rows[k];
      if (row[es::kNalLength] > 0) type = row[es::kNalType];
    }
    const unsigned long long m7 = __ballot(type == 7), m8 = __ballot(type == 8);
    if (lane == 0) {
      if (m7) atomicMin(&s_found[es::kPsSps], kb + wave * 64 + __builtin_ctzll(m7));
      if (m8) atomicMin(&s_found[es::kPsPps], kb + wave * 64 + __builtin_ctzll(m8));
    }
    __syncthreads();
    const bool done = s_found[es::kPsSps] != kCcNone && s_found[es::kPsPps] != kCcNone;
    __syncthreads();  // every wave has read the round's result before the next round may change it
    if (done) break;
  }
  const int found[es::kPsRows] = {s_found[es::kPsSps], s_found[es::kPsPps]};

  // ---- b. both NAL units to ps, the SPS to LDS as well
  int len[es::kPsRows] = {0, 0}, src[es::kPsRows] = {0, 0};
#pragma unroll
  for (int w = 0; w < es::kPsRows; ++w) {
    if (found[w] == kCcNone) continue;
    const v4i row = rows[found[w]];
    src[w] = static_cast<int>(clamp(row[es::kNalOffset], 0, cap_es));
    len[w] = static_cast<int>(clamp(row[es::kNalLength], 0, cap_es - src[w]));
  }
  if (wave < es::kPsRows && lane * 16 < max_ps) {
    const int64_t off = es_off[seg];
    const int64_t avail = es_numel - off;
    const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<uint8_t*>(es + off), 0, static_cast<int>(avail < 0x7fffffff ? avail : 0x7fffffff), 0x00020000);
    const int stored = len[wave] < max_ps ? len[wave] : max_ps;
    const int left = stored - lane * 16;  // bytes of this lane's 16 that are stored
    v4u q = {0, 0, 0, 0};
    if (left > 0) {
      const int sa = src[wave] + lane * 16;
      const v4u v = __builtin_amdgcn_raw_buffer_load_b128(rsrc, sa & ~3, 0, 0);
      const uint32_t w4 = __builtin_amdgcn_raw_buffer_load_b32(rsrc, (sa & ~3) + 16, 0, 0);
      const uint32_t sh = static_cast<uint32_t>(sa & 3);
      q = v4u{__builtin_amdgcn_alignbyte(v.y, v.x, sh), __builtin_amdgcn_alignbyte(v.z, v.y, sh),
              __builtin_amdgcn_alignbyte(v.w, v.z, sh), __builtin_amdgcn_alignbyte(w4, v.w, sh)};
#pragma unroll
      for (int d = 0; d < 4; ++d) {  // zero behind the stored bytes
        const int keep = left - 4 * d;
        if (keep <= 0) q[d] = 0;
        else if (keep < 4) q[d] &= (1u << (8 * keep)) - 1u;
      }
    }
    uint8_t* dst = ps_all + es::ps_bytes(seg, max_ps) + static_cast<int64_t>(wave) * max_ps;
    *reinterpret_cast<v4u*>(dst + lane * 16) = q;
    if (wave == es::kPsSps) *reinterpret_cast<v4u*>(s_raw + lane * 16) = q;
  }
  __syncthreads();

  // ---- c. the SPS without its header byte and emulation prevention
  const bool parse = found[es::kPsSps] != kCcNone && len[es::kPsSps] <= max_ps;  // an overflowed SPS is not parsed
  const int n = parse ? len[es::kPsSps] : 0;
  int carry = 0;
  for (int jb = 0; jb < n; jb += kCcThreads) {  // n is workgroup-uniform
    const int j = jb + tid;
    bool keep = false;
    uint8_t b = 0;
    if (j >= 1 && j < n) {
      b = s_raw[j];
      keep = j < 2 || !es::is_emulation_prevention(s_raw[j - 2], s_raw[j - 1], b);
    }
    const unsigned long long m = __ballot(keep);
    if (lane == 0) s_wave[wave] = __popcll(m);
    __syncthreads();
    int before = carry, total = 0;
#pragma unroll
    for (int w = 0; w < kCcWaves; ++w) {
      if (w < wave) before += s_wave[w];
      total += s_wave[w];
    }
    if (keep) s_rbsp[before + __popcll(m & ((1ull << lane) - 1ull))] = b;
    carry += total;
    __syncthreads();  // s_wave is free again
  }

  // ---- d. one lane parses, one of another wave takes the ADTS fields
  if (tid == 0) {
    int32_t status = 0;
    if (!avc) status |= es::kConfigUnsupportedVideo;
    else status |= (found[es::kPsSps] == kCcNone ? es::kNoSps : 0) | (found[es::kPsPps] == kCcNone ? es::kNoPps : 0);
    if (len[es::kPsSps] > max_ps || len[es::kPsPps] > max_ps) status |= es::kPsOverflow;
    s_row[es::kCSpsNal] = found[es::kPsSps] == kCcNone ? -1 : found[es::kPsSps];
    s_row[es::kCPpsNal] = found[es::kPsPps] == kCcNone ? -1 : found[es::kPsPps];
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
    if (audio.n_adts >= 1 && ix.aframes[es::kApesFrames] >= 1) {
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
  hipLaunchKernelGGL(codec_config_kernel, dim3(b.nseg), dim3(kCcThreads), 0, b.stream, b.es, b.es_numel, b.es_off,
                     b.cap, b.info, b.pes, b.max_pes, b.max_nal, b.ix.nal, b.ix.au, b.ix.aframes, b.ix.sinfo,
                     static_cast<int>(a.max_ps), a.ps, a.cinfo);
  return hipGetLastError();
}

}  // namespace dev
}  // namespace hlsp2p
