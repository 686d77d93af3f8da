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
// No workgroup waits for another one: the order comes from the launches alone.
#include "remux_dev.h"

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

// ---------------------------------------------------------------- 1. plan
// Separate `__restrict__` parameters, as remux_plan_kernel takes them and for the same reason.
__global__ __launch_bounds__(kRxThreads) void mpa_plan_kernel(
    const uint8_t* __restrict__ es, int64_t es_numel, const int64_t* __restrict__ es_off,
    const int64_t* __restrict__ cap, const int64_t* __restrict__ info, const int64_t* __restrict__ pes, int64_t max_pes,
    const int64_t* __restrict__ region_all, int64_t max_aframes, int32_t* __restrict__ scratch,
    int32_t* __restrict__ mf_all, int64_t* __restrict__ mpainfo, int32_t* __restrict__ as_all,
    int64_t* __restrict__ rinfo, uint8_t* __restrict__ out, const int64_t* __restrict__ out_off) {
  __shared__ int64_t s_w[kRxWaves];
  __shared__ int s_nrec, s_q, s_flags;
  const int seg = blockIdx.x;
  const int tid = threadIdx.x;
  const EsBatchView b{es, es_numel, es_off, cap, info, pes, max_pes, 0, {nullptr, nullptr, nullptr, nullptr}};
  const es::Segment sg = es_segment_clamped(b, seg);
  int32_t* mf = mf_all + table_words(seg, max_pes, es::kApesWords);
  int64_t* mi = mpainfo + static_cast<int64_t>(seg) * es::kMpainfoWords;
  const es::MpaScratch part = es::mpa_scratch(1, max_pes);
  int32_t* sc = scratch + static_cast<int64_t>(seg) * part.stride;
  const bool mpa = es::is_mpeg_audio(sg.info[ts::kAudioType]);
  const es::AudioSpan audio = es::audio_span(sg);
  const int64_t n = audio.n_pes;
  const int64_t* ap = es::pes_rows(sg).audio;
  const MpaFrameAt frame_at = {es_segment_rsrc(b, seg), static_cast<int>(audio.off)};

  // ---- every lane: the frame at the start of PES 0 gives the segment's key
  es::MpaFrame first = {0, false, 0, 0, 0, 0, 0, 0, 0};
  if (mpa && n > 0) {
    const es::ByteRange r0 = es::mpa_pes_range(ap, 0, audio);
    first = frame_at(r0.start, r0.end);
  }
  if (!first.counts) {  // workgroup-uniform: the fill values, nothing of the remux's is touched
    for (int64_t a = tid; a < max_pes; a += kRxThreads) {
      mf[es::kApesWords * a + es::kApesFrames] = -1;
      mf[es::kApesWords * a + es::kApesUsed] = -1;
    }
    if (tid < es::kMpainfoWords) mi[tid] = tid != es::kMpStatus ? 0 : mpa ? es::kMpaNoAudioConfig : es::kMpaNotMpegAudio;
    if (tid == 0) sc[0] = 0;
    return;
  }
  if (tid == 0) {
    s_nrec = 0;
    s_q = 0;
    s_flags = 0;
  }
  for (int64_t a = n + tid; a < max_pes; a += kRxThreads) {
    mf[es::kApesWords * a + es::kApesFrames] = -1;
    mf[es::kApesWords * a + es::kApesUsed] = -1;
  }
  __syncthreads();  // the shared words are set

  int64_t* ri = rinfo + static_cast<int64_t>(seg) * es::kRinfoWords;
  int32_t* as = as_all + table_words(seg, max_aframes, es::kAsampleWords);
  int32_t* pstart = sc + part.pstart;
  int32_t* psrc = sc + part.psrc;
  const int64_t region = region_all[seg];
  const int64_t A0 = es::mpa_audio_box(ri[es::kAudioBoxOffset], region);
  const int64_t room = region - (A0 + 8);
  const int32_t key = first.key;

  // ---- a lane per audio PES, a carry across rounds of the workgroup: two walks around two scans
  int64_t fcarry = 0, bcarry = 0;
  for (int64_t kb = 0; kb < n; kb += kRxThreads) {  // n is workgroup-uniform
    const int64_t k = kb + tid;
    int64_t start = 0, end = 0;
    es::MpaWalk w = {0, 0, false, false};
    if (k < n) {
      const es::ByteRange r = es::mpa_pes_range(ap, k, audio);
      start = r.start;
      end = r.end;
      w = es::mpa_walk(frame_at, start, end, key, [](int32_t, int64_t, int32_t) {});
      mf[es::kApesWords * k + es::kApesFrames] = w.frames;
      mf[es::kApesWords * k + es::kApesUsed] = w.used;
    }
    int64_t ftotal, btotal;
    int64_t fi = fcarry + rx_block_scan(static_cast<int64_t>(w.frames), s_w, ftotal);
    int64_t bo = bcarry + rx_block_scan(static_cast<int64_t>(w.used), s_w, btotal);
    fcarry += ftotal;
    bcarry += btotal;
    if (k < n) {
      pstart[k] = rx_sat32(bo);
      psrc[k] = static_cast<int32_t>(audio.off + start);
    }
    int nrec = 0, qsum = 0;
    bool over = false;
    int64_t q = start;
    for (int32_t j = 0; j < w.frames; ++j, ++fi) {
      const int64_t len = frame_at(q, end).len;
      if (fi < max_aframes && bo + len <= room) {  // a prefix of the frames: both sides only grow
        as[es::kAsampleWords * fi + es::kAsOffset] = static_cast<int32_t>(bo);
        as[es::kAsampleWords * fi + es::kAsSize] = static_cast<int32_t>(len);
        ++nrec;
        qsum += static_cast<int>(len);
      } else {
        over = true;
      }
      bo += len;
      q += len;
    }
    if (nrec) {
      atomicAdd(&s_nrec, nrec);
      atomicAdd(&s_q, qsum);
    }
    const int flags = (w.error ? es::kMpaError : 0) | (w.format_change ? es::kMpaFormatChange : 0) |
                      (over ? es::kMpaAframeOverflow : 0);
    if (flags) atomicOr(&s_flags, flags);
  }
  __syncthreads();
  const int64_t Q = s_q;

  // ---- totals and the box header
  uint8_t* o = out + out_off[seg];
  if (tid < 8) {
    const uint32_t word = tid < 4 ? static_cast<uint32_t>(8 + Q) : 0x6d646174u;  // 'mdat'
    o[A0 + tid] = static_cast<uint8_t>(word >> (8 * (3 - (tid & 3))));
  }
  if (tid == 0) {
    pstart[n] = rx_sat32(bcarry);
    sc[0] = static_cast<int32_t>(n);
    const int64_t status = s_flags;
    ri[es::kAudioPayloadBytes] = Q;
    ri[es::kNumAframes] = fcarry;
    if (status & es::kMpaAframeOverflow) ri[es::kRStatus] |= es::kAframeOverflow;
    mi[es::kMpStatus] = status;
    mi[es::kMpNumFrames] = fcarry;
    mi[es::kMpSampleRate] = first.rate;
    mi[es::kMpChannels] = first.channels;
    mi[es::kMpVersion] = first.version;
    mi[es::kMpLayer] = first.layer;
    mi[es::kMpFrameSamples] = first.samples;
    mi[es::kMpBitrate] = first.bitrate;
  }
}

// ---------------------------------------------------------------- 2. copy
__global__ __launch_bounds__(kRxThreads) void mpa_copy_kernel(
    EsBatchView b, const int64_t* __restrict__ tile_prefix, int nseg, const int32_t* __restrict__ scratch,
    const int64_t* __restrict__ rinfo, const int64_t* __restrict__ mpainfo, const int64_t* __restrict__ region_all,
    uint8_t* __restrict__ out, const int64_t* __restrict__ out_off) {
  const int64_t gt = blockIdx.x;
  const int seg = find_seg_wave(tile_prefix, nseg, gt);
  const int b0 = static_cast<int>(gt - tile_prefix[seg]) * es::kRemuxTile;
  if (mpainfo[static_cast<int64_t>(seg) * es::kMpainfoWords + es::kMpStatus] & (es::kMpaNotMpegAudio | es::kMpaNoAudioConfig))
    return;  // the plan wrote nothing for the segment
  const int64_t* ri = rinfo + static_cast<int64_t>(seg) * es::kRinfoWords;
  const int A0 = static_cast<int>(es::mpa_audio_box(ri[es::kAudioBoxOffset], region_all[seg]));
  const int Q = static_cast<int>(ri[es::kAudioPayloadBytes]);
  if (b0 >= A0 + 8 + Q || b0 + es::kRemuxTile <= A0 + 8) return;  // no payload byte in this tile
  const es::MpaScratch part = es::mpa_scratch(1, b.max_pes);
  const int32_t* sc = scratch + static_cast<int64_t>(seg) * part.stride;
  const __amdgpu_buffer_rsrc_t rsrc = es_segment_rsrc(b, seg);
  rx_copy_stream<0>(rsrc, b.es + b.es_off[seg], out + out_off[seg], b0, A0 + 8, A0 + 8 + Q, sc + part.pstart,
                    sc + part.psrc, sc[0]);
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
