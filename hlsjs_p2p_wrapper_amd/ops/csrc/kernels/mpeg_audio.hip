// MPEG audio (MPEG-1/2/2.5 Layer I-III) tracks of demuxed TS segments, behind the remux
// (docs/MPEGAUDIO.md) — CDNA4 / gfx950.
//
// Input: what ts_demux.hip leaves in HBM (es, info, pes) and what remux.hip wrote for the segment
// (rinfo's audio box offset; an empty audio mdat and -1 asamples rows, since the remux walks ADTS
// only).  Output per segment, identical to the host implementation runtime/mpegaudio.cpp
// mpeg_audio_segment:
//   mframes:  int32[seg][max_pes][kApesWords]  (whole frames, and their bytes; -1 rows beyond)
//   mpainfo:  int64[seg][kMpainfoWords]
//   asamples: the recorded frames' rows (offset, size), rinfo: Q, the frame total, the overflow bit
//   out:      at out_off[seg] + A0 the 'mdat' box of the whole frames, headers included
// A segment of any other audio type, or without a counting frame at the start of audio PES 0, gets
// the fill values and keeps every byte of asamples, rinfo and out.
//
// Two launches on the caller's stream, launched for every batch because the codec is only known on
// the device; no host round trip (host caps size the tile space and bound every access):
//   1. mpa_plan_kernel — one workgroup per segment.  Every lane reads the header at the start of
//                        PES 0 for the segment's key; a lane per audio PES walks its frames (a
//                        chain of dependent 4-byte reads through a buffer range that ends with the
//                        ES tensor), two workgroup scans with a carry give each PES its first
//                        frame rank and payload offset, a second walk writes the asamples rows.
//                        Frames are whole and back to back, so the copy needs one scratch row per
//                        PES: payload start and source offset.
//   2. mpa_copy_kernel — output-driven, remux_dev.h rx_copy_stream with a PES per row: one
//                        workgroup per 16 KiB tile of the region, a lane per 16 aligned output
//                        bytes, tiles outside [A0 + 8, A0 + 8 + Q) exit at once.
// No workgroup waits for another one: the order comes from the launches alone.  The bodies of both
// kernels are audio_frames_dev.h's templates, shared with ac3_audio.hip; this file is the MPEG audio rule.
#include "audio_frames_dev.h"

namespace hlsp2p {
namespace dev {

int mpeg_audio_tile_bytes() { return es::kRemuxTile; }

// es::mpa_frame_at on the audio ES at a_off of a segment's buffer range: bytes [q, q + 4) come from
// two aligned dwords, and a dword outside the ES tensor reads 0
struct MpaFrameAt {
  __amdgpu_buffer_rsrc_t rsrc;
  int a_off;
  __device__ __forceinline__ es::MpaFrame operator()(int64_t q, int64_t end) const {
    if (q + 4 > end) return {0, false, 0, 0, 0, 0, 0, 0, 0};
    const int off = a_off + static_cast<int>(q);
    const uint32_t lo = __builtin_amdgcn_raw_buffer_load_b32(rsrc, off & ~3, 0, 0);
    const uint32_t hi = __builtin_amdgcn_raw_buffer_load_b32(rsrc, (off & ~3) + 4, 0, 0);
    const uint32_t w = __builtin_amdgcn_alignbyte(hi, lo, static_cast<uint32_t>(off & 3));
    if ((w & 0xff) != 0xFF) return {0, false, 0, 0, 0, 0, 0, 0, 0};
    es::MpaFrame f = es::mpa_header((w >> 8) & 0xff, (w >> 16) & 0xff, w >> 24);
    f.counts = f.len > 0 && q + f.len <= end;
    return f;
  }
};

// The MPEG audio rule of audio_frames_dev.h: one info table, mpainfo.
struct MpaRule {
  using Frame = es::MpaFrame;
  using FrameAt = MpaFrameAt;
  struct Out { int64_t* mpainfo; };
  static constexpr int kInfoWords = es::kMpainfoWords;
  static constexpr int kError = es::kMpaError, kFormatChange = es::kMpaFormatChange, kAframeOverflow = es::kMpaAframeOverflow;
  static __device__ __forceinline__ bool mine(int64_t atype) { return es::is_mpeg_audio(atype); }
  static __device__ __forceinline__ Frame none() { return {0, false, 0, 0, 0, 0, 0, 0, 0}; }
  static __device__ __forceinline__ void fill(const Out& o, int seg, int tid, bool mpa, const Frame&) {
    int64_t* mi = o.mpainfo + static_cast<int64_t>(seg) * es::kMpainfoWords;
    if (tid < es::kMpainfoWords) mi[tid] = tid != es::kMpStatus ? 0 : mpa ? es::kMpaNoAudioConfig : es::kMpaNotMpegAudio;
  }
  static __device__ __forceinline__ void write(const Out& o, int seg, int64_t status, int64_t n_frames, const Frame& first) {
    int64_t* mi = o.mpainfo + static_cast<int64_t>(seg) * es::kMpainfoWords;
    mi[es::kMpStatus] = status;
    mi[es::kMpNumFrames] = n_frames;
    mi[es::kMpSampleRate] = first.rate;
    mi[es::kMpChannels] = first.channels;
    mi[es::kMpVersion] = first.version;
    mi[es::kMpLayer] = first.layer;
    mi[es::kMpFrameSamples] = first.samples;
    mi[es::kMpBitrate] = first.bitrate;
  }
};

// ---------------------------------------------------------------- 1. plan
// Separate `__restrict__` parameters, as remux_plan_kernel takes them and for the same reason.
__global__ __launch_bounds__(kRxThreads) void mpa_plan_kernel(
    const uint8_t* __restrict__ es, int64_t es_numel, const int64_t* __restrict__ es_off,
    const int64_t* __restrict__ cap, const int64_t* __restrict__ info, const int64_t* __restrict__ pes, int64_t max_pes,
    const int64_t* __restrict__ region_all, int64_t max_aframes, int32_t* __restrict__ scratch,
    int32_t* __restrict__ mf_all, int64_t* __restrict__ mpainfo, int32_t* __restrict__ as_all,
    int64_t* __restrict__ rinfo, uint8_t* __restrict__ out, const int64_t* __restrict__ out_off) {
  audio_plan_body<MpaRule>(es, es_numel, es_off, cap, info, pes, max_pes, region_all, max_aframes, scratch, mf_all,
                           MpaRule::Out{mpainfo}, as_all, rinfo, out, out_off);
}

// ---------------------------------------------------------------- 2. copy
__global__ __launch_bounds__(kRxThreads) void mpa_copy_kernel(
    EsBatchView b, const int64_t* __restrict__ tile_prefix, int nseg, const int32_t* __restrict__ scratch,
    const int64_t* __restrict__ rinfo, const int64_t* __restrict__ mpainfo, const int64_t* __restrict__ region_all,
    uint8_t* __restrict__ out, const int64_t* __restrict__ out_off) {
  audio_copy_body<MpaRule>(b, tile_prefix, nseg, scratch, rinfo, mpainfo, region_all, out, out_off);
}

hipError_t launch_mpeg_audio(const MpegAudioArgs& a) {
  const EsBatch& b = a.b;
  if (b.nseg <= 0) return hipSuccess;
  hipLaunchKernelGGL(mpa_plan_kernel, dim3(b.nseg), dim3(kRxThreads), 0, b.stream, b.es, b.es_numel, b.es_off, b.cap,
                     b.info, b.pes, b.max_pes, a.region, a.max_aframes, a.scratch, a.t.mframes, a.t.mpainfo,
                     a.t.asamples, a.t.rinfo, a.out, a.out_off);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess || b.total_tiles <= 0) return e;
  hipLaunchKernelGGL(mpa_copy_kernel, dim3(static_cast<unsigned>(b.total_tiles)), dim3(kRxThreads), 0, b.stream,
                     es_batch_view(b), b.tile_prefix, b.nseg, a.scratch, a.t.rinfo, a.t.mpainfo, a.region, a.out,
                     a.out_off);
  return hipGetLastError();
}

}  // namespace dev
}  // namespace hlsp2p
