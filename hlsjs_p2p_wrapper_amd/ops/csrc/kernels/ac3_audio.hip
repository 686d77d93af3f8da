// AC-3 / E-AC-3 tracks of demuxed TS segments, behind the remux (docs/AC3AUDIO.md) — CDNA4 / gfx950.
//
// Input: what ts_demux.hip leaves in HBM (es, info, pes) and what remux.hip wrote for the segment
// (rinfo's audio box offset; an empty audio mdat and -1 asamples rows, since the remux walks ADTS
// only), and optionally the mpainfo rows of mpeg_audio.hip.  Output per segment, identical to the
// host implementation runtime/ac3audio.cpp ac3_audio_segment:
//   dframes:  int32[seg][max_pes][kApesWords]  (whole syncframes, and their bytes; -1 rows beyond)
//   ac3info:  int64[seg][kAc3infoWords]
//   mpainfo:  int64[seg][kMpainfoWords]  (the row fragment_moof takes: the Dolby track's rate and
//             frame samples, else a copy of the MPEG audio op's row, else "not MPEG audio")
//   asamples: the recorded frames' rows (offset, size), rinfo: Q, the frame total, the overflow bit
//   out:      at out_off[seg] + A0 the 'mdat' box of the whole syncframes
// A segment of any other audio type, or without a counting frame at the start of audio PES 0, gets
// the fill values and keeps every byte of asamples, rinfo and out.
//
// Two launches on the caller's stream, as mpeg_audio.hip makes them and with the same bodies
// (audio_frames_dev.h): ac3_plan_kernel, one workgroup per segment and a lane per audio PES, and
// ac3_copy_kernel, output-driven with a PES per row.  This file is the Dolby rule: the 7 header bytes
// at any byte offset come from three aligned dwords of the segment's buffer range, where a dword
// outside the ES tensor reads 0, funnelled with v_alignbyte.  No workgroup waits for another one.
#include "audio_frames_dev.h"

namespace hlsp2p {
namespace dev {

int ac3_audio_tile_bytes() { return es::kRemuxTile; }

// es::ac3_frame_at on the audio ES at a_off of a segment's buffer range
struct Ac3FrameAt {
  __amdgpu_buffer_rsrc_t rsrc;
  int a_off;
  __device__ __forceinline__ es::Ac3Frame operator()(int64_t q, int64_t end) const {
    const es::Ac3Frame none = {0, false, es::kAc3NoKey, false, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    if (q + 7 > end) return none;  // before the bytes are trusted
    const int off = a_off + static_cast<int>(q);
    const uint32_t d0 = __builtin_amdgcn_raw_buffer_load_b32(rsrc, off & ~3, 0, 0);
    const uint32_t d1 = __builtin_amdgcn_raw_buffer_load_b32(rsrc, (off & ~3) + 4, 0, 0);
    const uint32_t d2 = __builtin_amdgcn_raw_buffer_load_b32(rsrc, (off & ~3) + 8, 0, 0);
    const uint32_t sh = static_cast<uint32_t>(off & 3);
    const uint32_t w0 = __builtin_amdgcn_alignbyte(d1, d0, sh);  // bytes q .. q + 3
    const uint32_t w1 = __builtin_amdgcn_alignbyte(d2, d1, sh);  // bytes q + 4 .. q + 7
    if ((w0 & 0xffff) != 0x770B) return none;
    es::Ac3Frame f = es::ac3_header((w0 >> 16) & 0xff, w0 >> 24, w1 & 0xff, (w1 >> 8) & 0xff, (w1 >> 16) & 0xff);
    f.counts = f.layout_ok && q + f.len <= end;
    return f;
  }
};

// The Dolby rule of audio_frames_dev.h: ac3info, and a row in mpainfo's layout for fragment_moof.
struct Ac3Rule {
  using Frame = es::Ac3Frame;
  using FrameAt = Ac3FrameAt;
  struct Out {
    int64_t* ac3info;
    int64_t* mpainfo;
    const int64_t* mpa_in;  // or null
  };
  static constexpr int kInfoWords = es::kAc3infoWords;
  static constexpr int kError = es::kAc3Error, kFormatChange = es::kAc3FormatChange, kAframeOverflow = es::kAc3AframeOverflow;
  static __device__ __forceinline__ bool mine(int64_t atype) { return es::is_dolby_audio(atype); }
  static __device__ __forceinline__ Frame none() { return {0, false, es::kAc3NoKey, false, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}; }
  static __device__ __forceinline__ void fill(const Out& o, int seg, int tid, bool dolby, const Frame& first) {
    int64_t* ai = o.ac3info + static_cast<int64_t>(seg) * es::kAc3infoWords;
    int64_t* mi = o.mpainfo + static_cast<int64_t>(seg) * es::kMpainfoWords;
    const int64_t status = !dolby ? int64_t(es::kAc3NotDolbyAudio)
                                  : es::kAc3NoAudioConfig | (first.len > 0 && !first.layout_ok ? es::kAc3UnsupportedLayout : 0);
    if (tid < es::kAc3infoWords) ai[tid] = tid != es::kAcStatus ? 0 : status;
    if (tid < es::kMpainfoWords) {
      int64_t v = tid != es::kMpStatus ? 0 : dolby ? es::kMpaNoAudioConfig : es::kMpaNotMpegAudio;
      if (!dolby && o.mpa_in) v = o.mpa_in[static_cast<int64_t>(seg) * es::kMpainfoWords + tid];
      mi[tid] = v;
    }
  }
  static __device__ __forceinline__ void write(const Out& o, int seg, int64_t status, int64_t n_frames, const Frame& first) {
    es::ac3_info_row(o.ac3info + static_cast<int64_t>(seg) * es::kAc3infoWords, status, n_frames, first);
    es::ac3_mpainfo_row(o.mpainfo + static_cast<int64_t>(seg) * es::kMpainfoWords, n_frames, first);
  }
};

// ---------------------------------------------------------------- 1. plan
// Separate `__restrict__` parameters, as mpa_plan_kernel takes them.  mpainfo and mpa_in never alias:
// the op allocates mpainfo itself.
__global__ __launch_bounds__(kRxThreads) void ac3_plan_kernel(
    const uint8_t* __restrict__ es, int64_t es_numel, const int64_t* __restrict__ es_off,
    const int64_t* __restrict__ cap, const int64_t* __restrict__ info, const int64_t* __restrict__ pes, int64_t max_pes,
    const int64_t* __restrict__ region_all, int64_t max_aframes, int32_t* __restrict__ scratch,
    int32_t* __restrict__ df_all, int64_t* __restrict__ ac3info, int64_t* __restrict__ mpainfo,
    const int64_t* __restrict__ mpa_in, int32_t* __restrict__ as_all, int64_t* __restrict__ rinfo,
    uint8_t* __restrict__ out, const int64_t* __restrict__ out_off) {
  audio_plan_body<Ac3Rule>(es, es_numel, es_off, cap, info, pes, max_pes, region_all, max_aframes, scratch, df_all,
                           Ac3Rule::Out{ac3info, mpainfo, mpa_in}, as_all, rinfo, out, out_off);
}

// ---------------------------------------------------------------- 2. copy
__global__ __launch_bounds__(kRxThreads) void ac3_copy_kernel(
    EsBatchView b, const int64_t* __restrict__ tile_prefix, int nseg, const int32_t* __restrict__ scratch,
    const int64_t* __restrict__ rinfo, const int64_t* __restrict__ ac3info, const int64_t* __restrict__ region_all,
    uint8_t* __restrict__ out, const int64_t* __restrict__ out_off) {
  audio_copy_body<Ac3Rule>(b, tile_prefix, nseg, scratch, rinfo, ac3info, region_all, out, out_off);
}

hipError_t launch_ac3_audio(const Ac3AudioArgs& a) {
  const EsBatch& b = a.b;
  if (b.nseg <= 0) return hipSuccess;
  hipLaunchKernelGGL(ac3_plan_kernel, dim3(b.nseg), dim3(kRxThreads), 0, b.stream, b.es, b.es_numel, b.es_off, b.cap,
                     b.info, b.pes, b.max_pes, a.region, a.max_aframes, a.scratch, a.t.dframes, a.t.ac3info, a.t.mpainfo,
                     a.t.mpa_in, a.t.asamples, a.t.rinfo, a.out, a.out_off);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess || b.total_tiles <= 0) return e;
  hipLaunchKernelGGL(ac3_copy_kernel, dim3(static_cast<unsigned>(b.total_tiles)), dim3(kRxThreads), 0, b.stream,
                     es_batch_view(b), b.tile_prefix, b.nseg, a.scratch, a.t.rinfo, a.t.ac3info, a.region, a.out,
                     a.out_off);
  return hipGetLastError();
}

}  // namespace dev
}  // namespace hlsp2p
