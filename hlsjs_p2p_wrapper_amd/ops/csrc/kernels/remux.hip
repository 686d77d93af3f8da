// Remux of demuxed and indexed segments to fMP4 samples and mdat boxes (docs/REMUX.md) — CDNA4 /
// gfx950.
//
// Input: what ts_demux.hip and es_index.hip leave in HBM.  Output per segment, identical to the
// host implementation runtime/remux.cpp remux_segment:
//   vsamples: int32[seg][max_pes][kVsampleWords]      (VsampleRow: offset, size, duration, cts, flags; -1 rows beyond)
//   asamples: int32[seg][max_aframes][kAsampleWords]  (AsampleRow: offset, size; -1 rows beyond)
//   rinfo:    int64[seg][kRinfoWords]
//   out:      at out_off[seg]: 'mdat' box of the video payload (4-byte length + NAL bytes per
//             kept NAL), then at the next multiple of 16 (behind audio_gap free bytes, default
//             none: docs/FRAGMENT.md) the 'mdat' box of the ADTS frame bodies
//
// Two launches on the caller's stream, no host round trip (host caps size the tile space and
// bound every access):
//   1. remux_plan_kernel — one workgroup per segment: a lane per NAL row (kept or not, output
//                          bytes; a workgroup scan with a carry gives every kept NAL its payload
//                          offset, sample sizes add up with integer atomics), a lane per access
//                          unit (timestamps, flags, then offsets by a second scan), a lane per
//                          audio PES (two walks over its counted frames around a scan of the PES
//                          totals), then rinfo and both box headers.  The payload offsets and
//                          source offsets go to scratch for the copy.
//   2. remux_copy_kernel — output-driven: one workgroup per 16 KiB tile of one segment's output
//                          region, a lane per 16 aligned output bytes.  The lane finds the NAL
//                          (or frame) that covers its bytes by binary search of the payload
//                          offsets, narrowed to the rows the tile touches; 16 bytes inside one
//                          body are funnelled out of five source dwords (common.h funnel16) and stored
//                          as one vector, every other chunk goes byte by byte and stores only
//                          payload bytes.  Tiles past the real output exit at once.
// No workgroup waits for another one: the order comes from the launches alone.
// The keep rule, the ADTS frame rule and the timestamp differences are shared/grammar.hpp
// (namespace es), the same functions runtime/remux.cpp calls.
#include "remux_dev.h"

namespace hlsp2p {
namespace dev {

int remux_tile_bytes() { return es::kRemuxTile; }

// ---------------------------------------------------------------- 1. plan
// The batch arrives as separate parameters here and becomes a view in the kernel: only a kernel
// argument carries readonly and noalias, which keep the uniform loads behind the first global
// store scalar.  With the view by value this kernel takes 85 VGPRs (occupancy 5) against 75 (6).
// audio_gap (docs/FRAGMENT.md) rides as one more scalar: still 75 VGPRs, occupancy 6, no scratch.
__global__ __launch_bounds__(kRxThreads) void remux_plan_kernel(
    const uint8_t* __restrict__ es, const int64_t* __restrict__ es_off, const int64_t* __restrict__ cap,
    const int64_t* __restrict__ info, const int64_t* __restrict__ pes, int64_t max_pes, int64_t max_nal,
    const int32_t* __restrict__ nal_all, const int32_t* __restrict__ au_all, const int32_t* __restrict__ af_all,
    const int64_t* __restrict__ sinfo, int64_t max_aframes, int32_t* __restrict__ scratch,
    int32_t* __restrict__ vs_all, int32_t* __restrict__ as_all, int64_t* __restrict__ rinfo, uint8_t* __restrict__ out,
    const int64_t* __restrict__ out_off, int64_t audio_gap) {
  __shared__ int64_t s_w[kRxWaves];
  __shared__ unsigned long long s_first_unfit;  // payload offset of the first kept NAL without room
  __shared__ int s_bad, s_nrec, s_q, s_aover;
  const int seg = blockIdx.x;
  const int tid = threadIdx.x;
  // no buffer resource here: es_numel stays unused
  const EsBatchView b{es, 0, es_off, cap, info, pes, max_pes, max_nal, {nal_all, au_all, af_all, sinfo}};
  const auto c = es_segment(b, seg);  // the clamped cap: offsets inside the segment are kept in int32 scratch rows
  const es::Segment& sg = c.sg;
  const es::RemuxTables tb = es::remux_tables_at({vs_all, as_all, rinfo}, sg, max_aframes, seg);
  const int64_t* si = c.ix.sinfo;
  const int64_t room_es = sg.cap;
  const uint8_t* V = sg.es;
  const bool supported = c.video.supported, hevc = c.video.hevc;
  const int64_t R = c.R, m = c.m;  // the index's counts, not the demux's
  const es::PesRows rows = es::pes_rows(sg);
  const int64_t *vp = rows.video, *ap = rows.audio;
  const int32_t *nal = c.ix.nal, *au = c.ix.au, *af = c.ix.aframes;
  int32_t *vs = tb.vsamples, *as = tb.asamples;
  const es::RemuxScratch part = es::remux_scratch(1, max_nal, max_aframes);
  int32_t* sc = scratch + static_cast<int64_t>(seg) * part.stride;
  int32_t* vstart = sc + part.vstart;
  int32_t* vsrc = sc + part.vsrc;
  int32_t* astart = sc + part.astart;
  int32_t* asrc = sc + part.asrc;
  uint8_t* o = out + out_off[seg];
  const int64_t region = es::remux_out_bytes(room_es, max_nal) + audio_gap;
  const int64_t v_limit = es::remux_video_limit(room_es, max_nal);
  if (tid == 0) {
    s_first_unfit = ~0ull;
    s_bad = 0;
    s_nrec = 0;
    s_q = 0;
    s_aover = 0;
  }

  // ---- a lane per sample row: timestamps and flags, size 0 for the atomics below
  bool bad = false;
  for (int64_t a = tid; a < max_pes; a += kRxThreads) {
    int32_t r0 = -1, r1 = -1, r2 = -1, r3 = -1, r4 = -1;
    if (a < m) {
      es::Delta32 dur = {0, true};
      const int64_t dts = es::pes_at(vp, a, ts::kPesDts);
      if (a + 1 < m) dur = es::delta32(es::pes_at(vp, a + 1, ts::kPesDts), dts, true);
      else if (m > 1) dur = es::delta32(dts, es::pes_at(vp, a - 1, ts::kPesDts), true);
      const es::Delta32 cts = es::delta32(es::pes_at(vp, a, ts::kPesPts), dts, false);
      bad |= !dur.fits || !cts.fits;
      r0 = 0;
      r1 = 0;
      r2 = dur.v;
      r3 = cts.v;
      r4 = (au[es::kAuWords * a + es::kAuFlags] & es::kAuKeyframe) ? es::kSampleSync : es::kSampleNonSync;
    }
    int32_t* row = vs + a * es::kVsampleWords;
    row[es::kVsOffset] = r0;
    row[es::kVsSize] = r1;
    row[es::kVsDuration] = r2;
    row[es::kVsCts] = r3;
    row[es::kVsFlags] = r4;
  }
  for (int64_t f = tid; f < max_aframes; f += kRxThreads) {
    as[es::kAsampleWords * f + es::kAsOffset] = -1;
    as[es::kAsampleWords * f + es::kAsSize] = -1;
  }
  __syncthreads();  // rows and the shared words are set
  if (bad) atomicOr(&s_bad, 1);

  // ---- a lane per NAL row, a carry across rounds of the workgroup
  int64_t carry = 0;
  for (int64_t kb = 0; kb < R; kb += kRxThreads) {  // R is workgroup-uniform
    const int64_t k = kb + tid;
    int64_t ob = 0, s = 0, a = -1;
    if (k < R) {
      const int32_t* row = nal + es::kNalWords * k;
      s = clamp(row[es::kNalOffset], 0, room_es);
      const int64_t len = clamp(row[es::kNalLength], 0, room_es - s);
      a = row[es::kNalAu];
      if (a >= 0 && a < m && len > 0 && es::nal_kept(hevc, row[es::kNalType])) ob = 4 + len;
    }
    int64_t total;
    const int64_t d = carry + rx_block_scan(ob, s_w, total);
    carry += total;
    if (k < R) {
      vstart[k] = rx_sat32(d);
      vsrc[k] = static_cast<int32_t>(s);
      if (ob > 0) {
        if (d + ob <= v_limit) atomicAdd(&vs[a * es::kVsampleWords + es::kVsSize], static_cast<int32_t>(ob));
        else atomicMin(&s_first_unfit, static_cast<unsigned long long>(d));
      }
    }
  }
  __syncthreads();  // sizes and s_first_unfit are complete
  const bool v_cut = s_first_unfit != ~0ull;
  const int64_t P = v_cut ? static_cast<int64_t>(s_first_unfit) : carry;
  if (tid == 0) vstart[R] = rx_sat32(carry);

  // ---- sample offsets
  int64_t acarry = 0;
  for (int64_t ab = 0; ab < m; ab += kRxThreads) {
    const int64_t a = ab + tid;
    const int64_t sz = a < m ? vs[a * es::kVsampleWords + es::kVsSize] : 0;
    int64_t total;
    const int64_t off = acarry + rx_block_scan(sz, s_w, total);
    acarry += total;
    if (a < m) vs[a * es::kVsampleWords + es::kVsOffset] = static_cast<int32_t>(off);
  }

  // ---- audio: a lane per PES walks its counted frames, twice around the scan of the totals
  const int64_t A0 = es::audio_box_offset(P, audio_gap);
  const int64_t a_room = region - (A0 + 8);
  const es::AudioSpan audio = es::audio_span(sg);
  const int64_t ma = audio.n_adts, a_off = audio.off;
  const uint8_t* A = V + a_off;
  int64_t fcarry = 0, bcarry = 0;
  for (int64_t kb = 0; kb < ma; kb += kRxThreads) {
    const int64_t k = kb + tid;
    int64_t start = 0, end = 0, want = 0, cnt = 0, bytes = 0;
    if (k < ma) {
      const es::ByteRange r = es::audio_pes_range(ap, k, audio);
      start = r.start;
      end = r.end;
      want = af[es::kApesWords * k + es::kApesFrames];
      int64_t q = start;
      for (; cnt < want; ++cnt) {
        const es::AdtsFrame f = es::adts_frame_at(A, q, end);
        if (f.len == 0) break;
        bytes += f.len - f.hdr;
        q += f.len;
      }
    }
    int64_t ftotal, btotal;
    int64_t fi = fcarry + rx_block_scan(cnt, s_w, ftotal);
    int64_t bo = bcarry + rx_block_scan(bytes, s_w, btotal);
    fcarry += ftotal;
    bcarry += btotal;
    int nrec = 0, qsum = 0;
    bool over = false;
    int64_t q = start;
    for (int64_t j = 0; j < cnt; ++j, ++fi) {
      const es::AdtsFrame f = es::adts_frame_at(A, q, end);
      const int64_t size = f.len - f.hdr;
      if (fi < max_aframes && bo + size <= a_room) {  // a prefix of the frames: both sides only grow
        as[es::kAsampleWords * fi + es::kAsOffset] = static_cast<int32_t>(bo);
        as[es::kAsampleWords * fi + es::kAsSize] = static_cast<int32_t>(size);
        astart[fi] = static_cast<int32_t>(bo);
        asrc[fi] = static_cast<int32_t>(a_off + q + f.hdr);
        ++nrec;
        qsum += static_cast<int>(size);
      } else {
        over = true;
      }
      bo += size;
      q += f.len;
    }
    if (nrec) {
      atomicAdd(&s_nrec, nrec);
      atomicAdd(&s_q, qsum);
    }
    if (over) atomicOr(&s_aover, 1);
  }
  __syncthreads();
  const int64_t n_rec = s_nrec, Q = s_q;

  // ---- totals and the two box headers
  if (tid < 16) {
    const bool second = tid >= 8;
    const int b = tid & 7;
    const uint32_t size = static_cast<uint32_t>(8 + (second ? Q : P));
    const uint32_t word = b < 4 ? size : 0x6d646174u;  // 'mdat'
    o[(second ? A0 : 0) + b] = static_cast<uint8_t>(word >> (8 * (3 - (b & 3))));
  }
  if (tid == 0) {
    astart[n_rec] = static_cast<int32_t>(Q);
    sc[0] = static_cast<int32_t>(R);
    sc[1] = static_cast<int32_t>(n_rec);
    int64_t status = supported ? 0 : es::kRemuxUnsupportedVideo;
    if ((si[es::kStatus] & es::kNalOverflow) || v_cut) status |= es::kTruncated;
    if (s_aover) status |= es::kAframeOverflow;
    if (s_bad) status |= es::kBadTimestamps;
    int64_t* ri = tb.rinfo;
    ri[es::kRStatus] = status;
    ri[es::kVideoPayloadBytes] = P;
    ri[es::kNumVsamples] = m;
    ri[es::kAudioBoxOffset] = A0;
    ri[es::kAudioPayloadBytes] = Q;
    ri[es::kNumAframes] = fcarry;
    ri[es::kVideoBaseDts] = m > 0 ? es::pes_at(vp, 0, ts::kPesDts) : -1;
    ri[es::kAudioBasePts] = audio.n_pes > 0 ? es::pes_at(ap, 0, ts::kPesPts) : -1;
  }
}

// ---------------------------------------------------------------- 2. copy
__global__ __launch_bounds__(kRxThreads) void remux_copy_kernel(
    EsBatchView b, const int64_t* __restrict__ tile_prefix, int nseg, int64_t max_aframes,
    const int32_t* __restrict__ scratch, const int64_t* __restrict__ rinfo, uint8_t* __restrict__ out,
    const int64_t* __restrict__ out_off) {
  const int64_t gt = blockIdx.x;
  const int seg = find_seg_wave(tile_prefix, nseg, gt);
  const int b0 = static_cast<int>(gt - tile_prefix[seg]) * es::kRemuxTile;
  const int64_t* ri = rinfo + static_cast<int64_t>(seg) * es::kRinfoWords;
  const int P = static_cast<int>(ri[es::kVideoPayloadBytes]);
  const int A0 = static_cast<int>(ri[es::kAudioBoxOffset]);
  const int Q = static_cast<int>(ri[es::kAudioPayloadBytes]);
  if (b0 >= A0 + 8 + Q) return;  // past the real output (A0 + 8 >= 8 + P)
  const es::RemuxScratch part = es::remux_scratch(1, b.max_nal, max_aframes);
  const int32_t* sc = scratch + static_cast<int64_t>(seg) * part.stride;
  const __amdgpu_buffer_rsrc_t rsrc = es_segment_rsrc(b, seg);
  const uint8_t* V = b.es + b.es_off[seg];
  uint8_t* o = out + out_off[seg];
  rx_copy_stream<4>(rsrc, V, o, b0, 8, 8 + P, sc + part.vstart, sc + part.vsrc, sc[0]);
  rx_copy_stream<0>(rsrc, V, o, b0, A0 + 8, A0 + 8 + Q, sc + part.astart, sc + part.asrc, sc[1]);
}

hipError_t launch_remux(const RemuxArgs& a) {
  const EsBatch& b = a.b;
  if (b.nseg <= 0) return hipSuccess;
  const EsBatchView view = es_batch_view(b);
  hipLaunchKernelGGL(remux_plan_kernel, dim3(b.nseg), dim3(kRxThreads), 0, b.stream, b.es, b.es_off, b.cap, b.info,
                     b.pes, b.max_pes, b.max_nal, b.ix.nal, b.ix.au, b.ix.aframes, b.ix.sinfo, a.max_aframes, a.scratch,
                     a.t.vsamples, a.t.asamples, a.t.rinfo, a.out, a.out_off, a.audio_gap);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess || b.total_tiles <= 0) return e;
  hipLaunchKernelGGL(remux_copy_kernel, dim3(static_cast<unsigned>(b.total_tiles)), dim3(kRxThreads), 0, b.stream,
                     view, b.tile_prefix, b.nseg, a.max_aframes, a.scratch, a.t.rinfo, a.out, a.out_off);
  return hipGetLastError();
}

}  // namespace dev
}  // namespace hlsp2p
