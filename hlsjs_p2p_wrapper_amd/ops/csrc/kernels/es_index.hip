// Sample index of demuxed segments (docs/ESINDEX.md) — CDNA4 / gfx950.
//
// Input: what ts_demux.hip leaves in HBM (ES bytes, PES tables, info rows).  Output per
// segment, identical to the host implementation runtime/es.cpp index_segment:
//   nal:     int32[seg][max_nal][kNalWords]   (NalRow: offset, length, type, access unit; -1 rows beyond)
//   au:      int32[seg][max_pes][kAuWords]    (AuRow: first NAL, NAL count, flags, size; -1 rows beyond)
//   aframes: int32[seg][max_pes][kApesWords]  (ApesRow: ADTS frames, bytes consumed, per audio PES)
//   sinfo:   int64[seg][kSinfoWords]
//
// Four launches on the caller's stream, no host round trip (the video ES lengths come from
// the demux's info rows; host caps size the tile space and bound every access):
//   1. es_count_kernel  — one workgroup per 16 KiB tile of one segment's video ES: every lane
//                         tests the 16 start-code positions of its 16 bytes in registers
//                         (SWAR zero / one byte flags over the 16-byte load plus one dword of
//                         look-ahead); counts reduce in the wave, then through LDS.
//   2. es_prefix_kernel — one wave per segment: exclusive tile prefixes, n_nal, status.
//   3. es_emit_kernel   — the count's grid: recomputes the matches and writes the start-code
//                         position of rank tile prefix + earlier iterations + earlier waves +
//                         earlier lanes + bit order, for ranks <= max_nal (the NAL after the
//                         last recorded one ends it).
//   4. es_finish_kernel — one workgroup per segment: a lane per recorded NAL (length, type,
//                         access unit by binary search of the PES offsets), a lane per access
//                         unit (NAL range, flags), then wave 0 counts the keyframe units and
//                         walks the ADTS frames with a lane per audio PES.
// No workgroup waits for another one: the order comes from the launches alone.
// The codec, NAL-type and ADTS byte rules are shared/grammar.hpp (namespace es), the same
// functions runtime/es.cpp calls.
#include "es_dev.h"

namespace hlsp2p {
namespace dev {

constexpr int kEsThreads = 256;
constexpr int kEsIters = 4;
constexpr int kEsIterBytes = kEsThreads * 16;
constexpr int kEsTile = kEsIters * kEsIterBytes;  // 16 KiB
int es_index_tile_bytes() { return kEsTile; }

// bytes of video ES to index: 0 for an unsupported codec, never beyond the host cap
__device__ __forceinline__ int64_t es_video_len(const int64_t* __restrict__ inf, int64_t cap) {
  return es::video_span(inf, cap).len;
}

// 0x80 in every byte of x that is zero (exact: no carry leaves a byte)
__device__ __forceinline__ uint32_t es_zero_bytes(uint32_t x) {
  return ~(((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x | 0x7f7f7f7fu);
}

// Bit j set: a start code begins at byte b + j of the video ES (00 00 01 with the NAL header
// byte inside the n bytes).  The ES is read through the segment's buffer resource (es_dev.h
// es_segment_rsrc), which ends with the ES tensor, so a load can never leave it; bytes at or
// past n (audio, slack) may take part in the flags, and the limit below drops every position
// whose header byte is not inside.
__device__ __forceinline__ uint32_t es_match16(__amdgpu_buffer_rsrc_t rsrc, int b, int n) {
  const int lim = n - 3 - b;  // positions j < lim have b + j + 3 < n
  if (lim <= 0) return 0;
  const v4u v = __builtin_amdgcn_raw_buffer_load_b128(rsrc, b, 0, 0);
  const uint32_t w4 = __builtin_amdgcn_raw_buffer_load_b32(rsrc, b + 16, 0, 0);
  const uint32_t w[5] = {v.x, v.y, v.z, v.w, w4};
  uint32_t z[5], o[5];
#pragma unroll
  for (int k = 0; k < 5; ++k) {
    z[k] = es_zero_bytes(w[k]);
    o[k] = es_zero_bytes(w[k] ^ 0x01010101u);
  }
  uint32_t mask = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const uint32_t m = z[k] & __builtin_amdgcn_alignbyte(z[k + 1], z[k], 1) & __builtin_amdgcn_alignbyte(o[k + 1], o[k], 2);
    mask |= ((((m >> 7) & 0x01010101u) * 0x01020408u) >> 24) << (4 * k);  // byte flags -> 4 bits
  }
  return lim >= 16 ? mask : mask & ((1u << lim) - 1u);
}

struct EsTile {
  int seg;
  int n;     // video ES bytes to index
  int base;  // first byte of the tile
  __amdgpu_buffer_rsrc_t rsrc;
};

__device__ __forceinline__ EsTile es_tile(const EsBatchView& b, const int64_t* __restrict__ tile_prefix, int nseg) {
  EsTile t;
  const int64_t gt = blockIdx.x;
  t.seg = find_seg_wave(tile_prefix, nseg, gt);
  t.base = static_cast<int>(gt - tile_prefix[t.seg]) * kEsTile;
  t.n = static_cast<int>(es_video_len(b.info + static_cast<int64_t>(t.seg) * ts::kInfoWords, b.cap[t.seg]));
  t.rsrc = es_segment_rsrc(b, t.seg);
  return t;
}

// ---------------------------------------------------------------- 1. count
__global__ __launch_bounds__(kEsThreads) void es_count_kernel(EsBatchView b, const int64_t* __restrict__ tile_prefix,
                                                              int nseg, int32_t* __restrict__ tile_cnt) {
  __shared__ uint32_t s_cnt[kEsThreads / 64];
  const EsTile t = es_tile(b, tile_prefix, nseg);
  const int tid = threadIdx.x;
  uint32_t c = 0;
  if (t.base < t.n) {
#pragma unroll
    for (int it = 0; it < kEsIters; ++it) c += __popc(es_match16(t.rsrc, t.base + it * kEsIterBytes + tid * 16, t.n));
  }
  const uint32_t inc = wave_scan_dpp(c);
  if ((tid & 63) == 63) s_cnt[tid >> 6] = inc;
  __syncthreads();
  if (tid == 0) tile_cnt[blockIdx.x] = static_cast<int32_t>(s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3]);
}

// ---------------------------------------------------------------- 2. prefix
__global__ __launch_bounds__(64) void es_prefix_kernel(const int64_t* __restrict__ tile_prefix,
                                                       const int32_t* __restrict__ tile_cnt,
                                                       int32_t* __restrict__ tile_pre, const int64_t* __restrict__ info,
                                                       int64_t max_nal, int64_t* __restrict__ sinfo) {
  const int seg = blockIdx.x;
  const int lane = threadIdx.x;
  const int64_t t0 = tile_prefix[seg];
  const int64_t nt = tile_prefix[seg + 1] - t0;
  uint32_t carry = 0;
  for (int64_t tb = 0; tb < nt; tb += 64) {
    const int64_t t = tb + lane;
    const uint32_t v = t < nt ? static_cast<uint32_t>(tile_cnt[t0 + t]) : 0u;
    const uint32_t inc = wave_scan_dpp(v);
    if (t < nt) tile_pre[t0 + t] = static_cast<int32_t>(carry + inc - v);
    carry += static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(inc), 63));
  }
  if (lane == 0) {  // carry is wave-uniform
    int64_t* si = sinfo + static_cast<int64_t>(seg) * es::kSinfoWords;
    const int64_t* inf = info + static_cast<int64_t>(seg) * ts::kInfoWords;
    int64_t status = es::video_supported(inf[ts::kVideoType]) ? 0 : es::kUnsupportedVideo;
    if (static_cast<int64_t>(carry) > max_nal) status |= es::kNalOverflow;
    si[es::kStatus] = status;
    si[es::kNumNal] = carry;
  }
}

// ---------------------------------------------------------------- 3. emit
__global__ __launch_bounds__(kEsThreads) void es_emit_kernel(EsBatchView b, const int64_t* __restrict__ tile_prefix,
                                                             int nseg, const int32_t* __restrict__ tile_pre,
                                                             int32_t* __restrict__ pos) {
  __shared__ uint32_t s_w[kEsIters][kEsThreads / 64];
  const int64_t max_nal = b.max_nal;
  const EsTile t = es_tile(b, tile_prefix, nseg);
  if (t.base >= t.n) return;  // block-uniform
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  uint32_t m[kEsIters], inc[kEsIters];
#pragma unroll
  for (int it = 0; it < kEsIters; ++it) m[it] = es_match16(t.rsrc, t.base + it * kEsIterBytes + tid * 16, t.n);
#pragma unroll
  for (int it = 0; it < kEsIters; ++it) {
    inc[it] = wave_scan_dpp(__popc(m[it]));
    if (lane == 63) s_w[it][wave] = inc[it];
  }
  __syncthreads();
  int32_t* out = pos + static_cast<int64_t>(t.seg) * (max_nal + 1);
  int64_t before = tile_pre[blockIdx.x];  // start codes of earlier tiles, iterations and waves
#pragma unroll
  for (int it = 0; it < kEsIters; ++it) {
    int64_t r = before + inc[it] - __popc(m[it]);
    for (int w = 0; w < kEsThreads / 64; ++w) {
      if (w < wave) r += s_w[it][w];
      before += s_w[it][w];
    }
    const int b = t.base + it * kEsIterBytes + tid * 16;
    for (uint32_t mm = m[it]; mm != 0 && r <= max_nal; mm &= mm - 1, ++r) out[r] = b + __ffs(mm) - 1;
  }
}

// ---------------------------------------------------------------- 4. finish
// first k in [0, cnt) with pos[k] + 3 >= x (NAL starts ascend), cnt if none
__device__ __forceinline__ int es_first_nal_at(const int32_t* __restrict__ pos, int cnt, int64_t x) {
  int lo = 0, hi = cnt;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (static_cast<int64_t>(pos[mid]) + 3 >= x) hi = mid; else lo = mid + 1;
  }
  return lo;
}

using EsIndexView = EsBatchViewOf<int32_t, int64_t>;  // this kernel writes the four tables

// The view serves for its pointers only: no es_segment here (see the two comments below).
__global__ __launch_bounds__(kEsThreads) void es_finish_kernel(EsIndexView b, const int32_t* __restrict__ pos_all) {
  const int seg = blockIdx.x;
  const int tid = threadIdx.x;
  const int64_t max_pes = b.max_pes, max_nal = b.max_nal;
  // cap as the wrapper checked it
  const es::Segment sg = es::segment_at(b.es, b.es_off, b.cap, b.info, b.pes, max_pes, max_nal, seg);
  const es::IndexTables<int32_t, int64_t> tb = es::index_tables_at(b.ix, sg, seg);
  int64_t* si = tb.sinfo;
  const uint8_t* V = sg.es;
  const es::VideoSpan video = es::video_span(sg);
  const int64_t n = video.len;
  const int64_t n_nal = si[es::kNumNal];
  const int nn = static_cast<int>(n_nal < max_nal ? n_nal : max_nal);
  const bool hevc = video.hevc;
  const int m = static_cast<int>(es::video_rows(video, sg.info[ts::kNumVideoPes], max_pes));  // the demux's count: one unit per PES
  const es::PesRows rows = es::pes_rows(sg);
  const int64_t *vp = rows.video, *ap = rows.audio;
  const int32_t* pos = pos_all + static_cast<int64_t>(seg) * (max_nal + 1);
  int32_t *nal = tb.nal, *au = tb.au, *af = tb.aframes;

  // ---- a lane per NAL row
  for (int64_t k = tid; k < max_nal; k += kEsThreads) {
    int32_t r0 = -1, r1 = -1, r2 = -1, r3 = -1;
    if (k < nn) {
      const int64_t s = static_cast<int64_t>(pos[k]) + 3;
      int64_t e = n;
      if (k + 1 < n_nal) {  // rank k + 1 <= max_nal is recorded
        const int64_t p1 = pos[k + 1];
        const int64_t z1 = (p1 > 0 && V[p1 - 1] == 0) ? 1 : 0;
        e = p1 - z1 > s ? p1 - z1 : s;
      }
      const int hb = V[s];
      int a_lo = 0, a_hi = m;  // AU: largest a < m with offset <= s, else -1
      while (a_lo < a_hi) {
        const int mid = (a_lo + a_hi) >> 1;
        if (es::pes_at(vp, mid, ts::kPesEsOffset) <= s) a_lo = mid + 1; else a_hi = mid;
      }
      r0 = static_cast<int32_t>(s);
      r1 = static_cast<int32_t>(e - s);
      r2 = e == s ? -1 : es::nal_type(hevc, hb);
      r3 = a_lo - 1;
    }
    int32_t* row = nal + es::kNalWords * k;
    row[es::kNalOffset] = r0;
    row[es::kNalLength] = r1;
    row[es::kNalType] = r2;
    row[es::kNalAu] = r3;
  }
  __syncthreads();  // NAL rows of this segment are visible to the whole workgroup

  // ---- a lane per access unit row
  for (int64_t a = tid; a < max_pes; a += kEsThreads) {
    int32_t r0 = -1, r1 = -1, r2 = -1, r3 = -1;
    if (a < m) {
      const int64_t o = es::pes_at(vp, a, ts::kPesEsOffset);
      const int64_t o_next = a + 1 < m ? es::pes_at(vp, a + 1, ts::kPesEsOffset) : n;
      const int first = es_first_nal_at(pos, nn, o);
      const int end = a + 1 < m ? es_first_nal_at(pos, nn, o_next) : nn;
      int flags = 0;
      for (int k = first; k < end; ++k) flags |= es::nal_flags(hevc, nal[es::kNalWords * k + es::kNalType]);
      r1 = end > first ? end - first : 0;
      r0 = r1 > 0 ? first : -1;
      r2 = flags;
      r3 = static_cast<int32_t>(o_next - o);
    }
    int32_t* row = au + es::kAuWords * a;
    row[es::kAuFirstNal] = r0;
    row[es::kAuNalCount] = r1;
    row[es::kAuFlags] = r2;
    row[es::kAuSize] = r3;
  }
  __syncthreads();
  if (tid >= 64) return;

  // ---- wave 0: keyframe units, then the ADTS walk (a lane per audio PES)
  const int lane = tid;
  int n_key = 0, first_key = 0x7fffffff;
  for (int a = lane; a < m; a += 64) {
    if (au[es::kAuWords * a + es::kAuFlags] & es::kAuKeyframe) {
      ++n_key;
      if (a < first_key) first_key = a;
    }
  }
  const es::AudioSpan audio = es::audio_span(sg);
  const uint8_t* A = V + audio.off;
  int n_frames = 0, err = 0, rate = 0, chans = 0;
  for (int64_t k = lane; k < max_pes; k += 64) {
    int32_t frames = -1, used = -1;
    if (k < audio.n_adts) {
      const es::ByteRange r = es::audio_pes_range(ap, k, audio);
      const es::AdtsWalk w = es::adts_walk(A, r.start, r.end, k == 0, rate, chans);
      frames = w.frames;
      used = w.used;
      err |= w.error;
      n_frames += frames;
    }
    af[es::kApesWords * k + es::kApesFrames] = frames;
    af[es::kApesWords * k + es::kApesUsed] = used;
  }
  n_key = static_cast<int>(__builtin_amdgcn_readlane(static_cast<int>(wave_scan_dpp(n_key)), 63));
  n_frames = static_cast<int>(__builtin_amdgcn_readlane(static_cast<int>(wave_scan_dpp(n_frames)), 63));
  const bool any_err = __ballot(err != 0) != 0;
  for (int d = 32; d > 0; d >>= 1) {
    const int other = __shfl_xor(first_key, d);
    first_key = other < first_key ? other : first_key;
  }
  if (lane == 0) {  // rate / chans: lane 0 walked audio PES 0
    si[es::kStatus] |= any_err ? es::kAdtsError : 0;
    si[es::kNumAu] = m;
    si[es::kNumKeyframeAus] = n_key;
    si[es::kFirstKeyframeAu] = n_key > 0 ? first_key : -1;
    si[es::kNumAdtsFrames] = n_frames;
    si[es::kAudioSampleRate] = rate;
    si[es::kAudioChannels] = chans;
  }
}

hipError_t launch_es_index(const EsIndexArgs& args) {
  const EsBatch& a = args.b;
  if (a.nseg <= 0) return hipSuccess;
  const es::IndexScratch part = es::index_scratch(a.total_tiles, a.nseg, a.max_nal);
  int32_t* tile_cnt = args.scratch + part.tile_cnt;
  int32_t* tile_pre = args.scratch + part.tile_pre;
  int32_t* pos = args.scratch + part.pos;
  const dim3 tiles(static_cast<unsigned>(a.total_tiles));
  const EsBatchView view = es_batch_view(a);
  hipError_t e = hipSuccess;
  if (a.total_tiles > 0) {
    hipLaunchKernelGGL(es_count_kernel, tiles, dim3(kEsThreads), 0, a.stream, view, a.tile_prefix, a.nseg, tile_cnt);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(es_prefix_kernel, dim3(a.nseg), dim3(64), 0, a.stream, a.tile_prefix, tile_cnt, tile_pre, a.info,
                     a.max_nal, a.ix.sinfo);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  if (a.total_tiles > 0) {
    hipLaunchKernelGGL(es_emit_kernel, tiles, dim3(kEsThreads), 0, a.stream, view, a.tile_prefix, a.nseg, tile_pre,
                       pos);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(es_finish_kernel, dim3(a.nseg), dim3(kEsThreads), 0, a.stream,
                     es_batch_view<int32_t, int64_t>(a), pos);
  return hipGetLastError();
}

}  // namespace dev
}  // namespace hlsp2p
