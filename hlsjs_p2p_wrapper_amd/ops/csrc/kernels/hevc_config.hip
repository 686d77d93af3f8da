// HEVC configuration of demuxed and indexed segments for the hvc1 init segment
// (docs/INITSEGMENT.md) — CDNA4 / gfx950.
//
// Input: what ts_demux.hip and es_index.hip leave in HBM.  Output per segment, identical to the
// host implementation runtime/hevc.cpp hevc_config_segment:
//   hps:   uint8[seg][kHpsRows][max_ps]  (the first VPS, SPS and PPS NAL units as they are, zero beyond)
//   hinfo: int32[seg][kHinfoWords]       (Hinfo: status, rows, lengths, SPS fields)
//
// One launch on the caller's stream, one 256-thread workgroup per segment, static LDS, no scratch:
//   0. not HEVC   — the workgroup writes its row (not_hevc, no rows) and zeros to hps and exits.
//   a. row search — ps_find_rows for the types 32, 33 and 34: three ballots per round of 256 rows.
//   b. byte copy  — wave 0 the VPS, wave 1 the SPS, wave 2 the PPS through ps_copy_lane, one
//                   16-byte store to hps and, for the SPS, one to LDS.
//   c. unescape   — ps_unescape of the SPS behind its two header bytes.
//   d. parse      — lane 0 runs es::hevc_sps_parse on the RBSP.
//   e. row write  — a lane per hinfo word.
// Steps a, b and c are ps_dev.h, shared with codec_config.hip.  No workgroup waits for another
// one.  The emulation-prevention predicate and hevc_sps_parse are shared/grammar.hpp (namespace
// es), the same functions runtime/hevc.cpp calls.
#include "es_dev.h"
#include "ps_dev.h"

namespace hlsp2p {
namespace dev {

static_assert(es::kHpsRows <= kPsWaves, "a wave per parameter set");
static_assert(es::kHinfoWords <= kPsThreads, "a lane per hinfo word");

__global__ __launch_bounds__(kPsThreads) void hevc_config_kernel(EsBatchView b, int max_ps,
                                                                 uint8_t* __restrict__ hps_all,
                                                                 int32_t* __restrict__ hinfo_all) {
  __shared__ __attribute__((aligned(16))) uint8_t s_raw[es::kMaxPsLimit];   // the SPS as stored
  __shared__ __attribute__((aligned(16))) uint8_t s_rbsp[es::kMaxPsLimit];  // ... and without emulation prevention
  __shared__ int s_found[es::kHpsRows];
  __shared__ int s_wave[kPsWaves];
  __shared__ int32_t s_row[es::kHinfoWords];
  const int seg = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const es::Segment sg = es_segment_clamped(b, seg);
  uint8_t* hps = hps_all + es::hps_bytes(seg, max_ps);
  int32_t* hinfo = hinfo_all + static_cast<int64_t>(seg) * es::kHinfoWords;
  const bool copies = wave < es::kHpsRows && lane * 16 < max_ps;  // this lane holds 16 bytes of hps

  // ---- 0. any other codec (workgroup-uniform, in front of the first barrier)
  if (!es::is_hevc(sg.info[ts::kVideoType])) {
    if (copies) *reinterpret_cast<v4u*>(hps + static_cast<int64_t>(wave) * max_ps + lane * 16) = v4u{0, 0, 0, 0};
    if (tid < es::kHinfoWords)
      hinfo[tid] = tid == es::kHStatus ? static_cast<int32_t>(es::kHNotHevc)
                   : tid == es::kHVpsNal || tid == es::kHSpsNal || tid == es::kHPpsNal ? -1 : 0;
    return;
  }
  const auto c = es_segment(b, seg);
  const int cap_es = c.cap;
  const int R = static_cast<int>(c.R);
  if (tid < es::kHpsRows) s_found[tid] = kPsNone;
  if (tid < es::kHinfoWords) s_row[tid] = 0;
  __syncthreads();

  // ---- a. the first VPS, SPS and PPS rows
  const v4i* rows = reinterpret_cast<const v4i*>(c.ix.nal);  // a table row is 16 bytes of a 16-byte aligned table
  const int types[es::kHpsRows] = {es::kHevcVps, es::kHevcSps, es::kHevcPps};
  ps_find_rows(rows, R, types, s_found);
  const int found[es::kHpsRows] = {s_found[es::kHpsVps], s_found[es::kHpsSps], s_found[es::kHpsPps]};

  // ---- b. the three NAL units to hps, the SPS to LDS as well
  int len[es::kHpsRows] = {0, 0, 0}, src[es::kHpsRows] = {0, 0, 0};
#pragma unroll
  for (int w = 0; w < es::kHpsRows; ++w) {
    if (found[w] == kPsNone) continue;
    const v4i row = rows[found[w]];
    src[w] = static_cast<int>(clamp(row[es::kNalOffset], 0, cap_es));
    len[w] = static_cast<int>(clamp(row[es::kNalLength], 0, cap_es - src[w]));
  }
  if (copies) {
    const int mine_src = wave == 0 ? src[0] : wave == 1 ? src[1] : src[2];
    const int mine_len = wave == 0 ? len[0] : wave == 1 ? len[1] : len[2];
    const v4u q = ps_copy_lane(es_segment_rsrc(b, seg), mine_src, mine_len, max_ps, lane);
    *reinterpret_cast<v4u*>(hps + static_cast<int64_t>(wave) * max_ps + lane * 16) = q;
    if (wave == es::kHpsSps) *reinterpret_cast<v4u*>(s_raw + lane * 16) = q;
  }
  __syncthreads();

  // ---- c. the SPS without its two header bytes and emulation prevention
  const bool parse = found[es::kHpsSps] != kPsNone && len[es::kHpsSps] <= max_ps;  // an overflowed SPS is not parsed
  const int carry = ps_unescape(s_raw, parse ? len[es::kHpsSps] : 0, es::kHevcNalHeader, s_rbsp, s_wave);

  // ---- d. one lane parses
  if (tid == 0) {
    int32_t status = (found[es::kHpsVps] == kPsNone ? es::kHNoVps : 0) | (found[es::kHpsSps] == kPsNone ? es::kHNoSps : 0) |
                     (found[es::kHpsPps] == kPsNone ? es::kHNoPps : 0);
    if (len[es::kHpsVps] > max_ps || len[es::kHpsSps] > max_ps || len[es::kHpsPps] > max_ps) status |= es::kHPsOverflow;
    s_row[es::kHVpsNal] = found[es::kHpsVps] == kPsNone ? -1 : found[es::kHpsVps];
    s_row[es::kHSpsNal] = found[es::kHpsSps] == kPsNone ? -1 : found[es::kHpsSps];
    s_row[es::kHPpsNal] = found[es::kHpsPps] == kPsNone ? -1 : found[es::kHpsPps];
    s_row[es::kHVpsBytes] = len[es::kHpsVps];
    s_row[es::kHSpsBytes] = len[es::kHpsSps];
    s_row[es::kHPpsBytes] = len[es::kHpsPps];
    if (parse) {
      es::HevcSpsFields f;
      const uint8_t* p = s_rbsp;
      if (!es::hevc_sps_parse([p](int64_t i) { return p[i]; }, carry, f)) status |= es::kHBadSps;
      s_row[es::kHSpsRbspBytes] = carry;
      s_row[es::kHProfileSpace] = f.profile_space;
      s_row[es::kHTierFlag] = f.tier_flag;
      s_row[es::kHProfileIdc] = f.profile_idc;
      s_row[es::kHProfileCompat] = f.profile_compat;
      s_row[es::kHConstraintHi] = f.constraint_hi;
      s_row[es::kHConstraintLo] = f.constraint_lo;
      s_row[es::kHLevelIdc] = f.level_idc;
      s_row[es::kHNumTemporalLayers] = f.num_temporal_layers;
      s_row[es::kHTemporalIdNested] = f.temporal_id_nested;
      s_row[es::kHChromaFormatIdc] = f.chroma_format_idc;
      s_row[es::kHBitDepthLuma] = f.bit_depth_luma;
      s_row[es::kHBitDepthChroma] = f.bit_depth_chroma;
      s_row[es::kHWidth] = f.width;
      s_row[es::kHHeight] = f.height;
    }
    s_row[es::kHStatus] = status;
  }
  __syncthreads();

  // ---- e. the row
  if (tid < es::kHinfoWords) hinfo[tid] = s_row[tid];
}

hipError_t launch_hevc_config(const HevcConfigArgs& a) {
  const EsBatch& b = a.b;
  if (b.nseg <= 0) return hipSuccess;
  hipLaunchKernelGGL(hevc_config_kernel, dim3(b.nseg), dim3(kPsThreads), 0, b.stream, es_batch_view(b),
                     static_cast<int>(a.max_ps), a.hps, a.hinfo);
  return hipGetLastError();
}

}  // namespace dev
}  // namespace hlsp2p
