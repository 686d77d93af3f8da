// What mpeg_audio.hip and ac3_audio.hip share on the device: the plan and the copy of an audio
// track whose samples are whole, self-delimiting frames, back to back in every audio PES
// (docs/MPEGAUDIO.md, docs/AC3AUDIO.md), as templates over a codec rule.  A rule supplies
//   Frame                  the frame type of the codec's grammar rule: len, counts, key
//   FrameAt{rsrc, a_off}   functor (q, end) -> Frame on the audio ES at a_off of a segment's buffer range
//   Out                    the codec's info tables (pointers for the whole batch)
//   kInfoWords             words of a row of the table status() reads
//   kError / kFormatChange / kAframeOverflow   status bits of the walk
//   mine(atype)            the segment's audio type is this codec's
//   none()                 a Frame that is no header
//   fill(out, seg, tid, mine, first)   the info rows of a segment without a config (every thread calls it)
//   write(out, seg, status, n_frames, first)   the info rows of a segment with one (one thread calls it)
//   status(out)            the int64 table whose slot 0 of a row has bits 1 | 2 set for a segment the plan left alone
// The kernels themselves are instantiated in the two .hip files: their names and arguments are the
// launch contract.
#pragma once
#include "remux_dev.h"

namespace hlsp2p {
namespace dev {

constexpr int64_t kAudioNoConfigMask = 3;  // "not this codec" | "no audio config", in both codecs' status words

// ---------------------------------------------------------------- 1. plan
// One workgroup per segment.  Every lane reads the header at the start of PES 0 for the segment's
// key; a lane per audio PES walks its frames (a chain of dependent header reads through a buffer
// range that ends with the ES tensor), two workgroup scans with a carry give each PES its first
// frame rank and payload offset, a second walk writes the asamples rows.  Frames are whole and back
// to back, so the copy needs one scratch row per PES: payload start and source offset.
template <class Rule>
__device__ __forceinline__ void audio_plan_body(
    const uint8_t* __restrict__ es, int64_t es_numel, const int64_t* __restrict__ es_off,
    const int64_t* __restrict__ cap, const int64_t* __restrict__ info, const int64_t* __restrict__ pes, int64_t max_pes,
    const int64_t* __restrict__ region_all, int64_t max_aframes, int32_t* __restrict__ scratch,
    int32_t* __restrict__ mf_all, const typename Rule::Out& outs, int32_t* __restrict__ as_all,
    int64_t* __restrict__ rinfo, uint8_t* __restrict__ out, const int64_t* __restrict__ out_off) {
  __shared__ int64_t s_w[kRxWaves];
  __shared__ int s_nrec, s_q, s_flags;
  const int seg = blockIdx.x;
  const int tid = threadIdx.x;
  const EsBatchView b{es, es_numel, es_off, cap, info, pes, max_pes, 0, {nullptr, nullptr, nullptr, nullptr}};
  const es::Segment sg = es_segment_clamped(b, seg);
  int32_t* mf = mf_all + table_words(seg, max_pes, es::kApesWords);
  const es::MpaScratch part = es::mpa_scratch(1, max_pes);
  int32_t* sc = scratch + static_cast<int64_t>(seg) * part.stride;
  const bool mine = Rule::mine(sg.info[ts::kAudioType]);
  const es::AudioSpan audio = es::audio_span(sg);
  const int64_t n = audio.n_pes;
  const int64_t* ap = es::pes_rows(sg).audio;
  const typename Rule::FrameAt frame_at = {es_segment_rsrc(b, seg), static_cast<int>(audio.off)};

  // ---- every lane: the frame at the start of PES 0 gives the segment's key
  typename Rule::Frame first = Rule::none();
  if (mine && n > 0) {
    const es::ByteRange r0 = es::mpa_pes_range(ap, 0, audio);
    first = frame_at(r0.start, r0.end);
  }
  if (!first.counts) {  // workgroup-uniform: the fill values, nothing of the remux's is touched
    for (int64_t a = tid; a < max_pes; a += kRxThreads) {
      mf[es::kApesWords * a + es::kApesFrames] = -1;
      mf[es::kApesWords * a + es::kApesUsed] = -1;
    }
    Rule::fill(outs, seg, tid, mine, first);
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
    const int flags = (w.error ? Rule::kError : 0) | (w.format_change ? Rule::kFormatChange : 0) |
                      (over ? Rule::kAframeOverflow : 0);
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
    if (status & Rule::kAframeOverflow) ri[es::kRStatus] |= es::kAframeOverflow;
    Rule::write(outs, seg, status, fcarry, first);
  }
}

// ---------------------------------------------------------------- 2. copy
// Output-driven, rx_copy_stream with a PES per row: one workgroup per 16 KiB tile of the region, a
// lane per 16 aligned output bytes; tiles outside [A0 + 8, A0 + 8 + Q), and segments the plan left
// alone, exit at once.  `status` is the table Rule::status names.
template <class Rule>
__device__ __forceinline__ void audio_copy_body(
    const EsBatchView& b, const int64_t* __restrict__ tile_prefix, int nseg, const int32_t* __restrict__ scratch,
    const int64_t* __restrict__ rinfo, const int64_t* __restrict__ status, const int64_t* __restrict__ region_all,
    uint8_t* __restrict__ out, const int64_t* __restrict__ out_off) {
  const int64_t gt = blockIdx.x;
  const int seg = find_seg_wave(tile_prefix, nseg, gt);
  const int b0 = static_cast<int>(gt - tile_prefix[seg]) * es::kRemuxTile;
  if (status[static_cast<int64_t>(seg) * Rule::kInfoWords] & kAudioNoConfigMask) return;  // the plan wrote nothing for the segment
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

}  // namespace dev
}  // namespace hlsp2p
