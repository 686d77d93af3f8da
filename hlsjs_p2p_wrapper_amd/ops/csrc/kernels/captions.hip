// CEA-608/708 caption data of the SEI NAL units of demuxed and indexed segments
// (docs/CAPTIONS.md) — CDNA4 / gfx950.
//
// Input: what ts_demux.hip and es_index.hip leave in HBM, only read.  Output per segment, identical
// to the host implementation runtime/captions.cpp caption_segment:
//   ccsamples: int32[seg][max_cc][kCcRowWords]   ccpts: int64[seg][max_cc]
//   ccbytes:   uint8[seg][max_cc][kCcSlotBytes]  cc608: uint8[seg][max_cc][2][kCcFieldBytes]
//   ccinfo:    int64[seg][kCcInfoWords]
//
// Two launches on the caller's stream, ordered by the stream alone; no workgroup waits for another:
//   1. cc_scan_kernel — grid ceil(max_nal / 64) x nseg, 256 threads.  Every wave loads the chunk's
//      64 NAL rows, a lane per row (one 16-byte load), runs the candidate test and comes to the same
//      ballot; the chunk's candidates go to the four waves in turn, and a wave takes its own one by
//      one with no workgroup barrier (the next candidate's load in flight meanwhile): ps_copy_lane
//      brings the stored bytes (at most kCcNalBytes, 16 per lane) through the segment's buffer
//      resource (es_dev.h es_segment_rsrc: it ends with the ES tensor) into the wave's 1 KiB of
//      LDS, a ballot / popcount prefix compacts the RBSP into a second KiB, every lane runs
//      es::cc_find over it (wave-uniform, LDS broadcast reads), and on a match six lanes store the
//      sample's 96-byte slot into scratch.  Every row k < R gets its flag word.
//   2. cc_pack_kernel — one workgroup per segment.  A workgroup scan of the hit flags in rounds of
//      256 rows with a carry ranks the samples; the lane of a hit row moves its slot, splits the
//      608 pairs by field and writes its row; the pts go to LDS and, behind a barrier, a lane per
//      sample counts its presentation rank; then the fills beyond the recorded count and ccinfo.
// A disabled segment, another codec and a chunk past R leave cc_scan_kernel in front of any work;
// cc_pack_kernel computes the same R and reads no flag the scan did not write.
// The batch view and the head of both kernels (clamped cap, R rows, m access units) are es_dev.h.
// The candidate test, the emulation-prevention predicate, cc_find and the 608 pair rule are
// shared/grammar.hpp (namespace es), the same functions runtime/captions.cpp calls.
#include "es_dev.h"
#include "ps_dev.h"

namespace hlsp2p {
namespace dev {

constexpr int kCcThreads = 256;
constexpr int kCcWaves = kCcThreads / 64;
constexpr int kCcChunkRows = 64;  // NAL rows per scan workgroup: a lane per row in every wave
static_assert(es::kCcNalBytes == 64 * 16, "a wave copies a candidate's stored bytes, a lane per 16");
static_assert(es::kCcSlotBytes % 16 == 0 && es::kCcSlotBytes >= 2 + 3 * es::kCcMaxTriples, "16-byte stores of a slot");
static_assert(2 * es::kCcMaxTriples <= es::kCcFieldBytes && es::kCcFieldBytes % 16 == 0, "a field's pairs fit its row");
static_assert(es::kCcRowWords == 8, "a ccsamples row is two 16-byte vectors");
static_assert(es::kMaxCcLimit * 8 <= 16384, "the pts of a segment's samples fit 16 KiB of LDS");

// the wave's LDS stores are visible to its own lanes behind this
__device__ __forceinline__ void cc_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__global__ __launch_bounds__(kCcThreads) void cc_scan_kernel(EsBatchView b, const uint8_t* __restrict__ enable,
                                                             int32_t* __restrict__ flag_all,
                                                             uint8_t* __restrict__ hit_all) {
  __shared__ __attribute__((aligned(16))) uint8_t s_raw[kCcWaves][es::kCcNalBytes];  // a candidate as stored
  __shared__ __attribute__((aligned(16))) uint8_t s_rbsp[kCcWaves][es::kCcNalBytes];  // ... behind its header, unescaped
  const int seg = blockIdx.y, chunk = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (!enable[seg]) return;
  const auto c = es_segment(b, seg);
  const int R = static_cast<int>(c.R), m = static_cast<int>(c.m);
  const bool hevc = c.video.hevc;
  if (chunk * kCcChunkRows >= R) return;
  const int h = es::nal_header_bytes(hevc);
  const v4i* rows = reinterpret_cast<const v4i*>(c.ix.nal);  // a table row is 16 bytes of a 16-byte aligned table
  int32_t* flag_seg = flag_all + static_cast<int64_t>(seg) * b.max_nal;
  uint8_t* hit_seg = hit_all + static_cast<int64_t>(seg) * b.max_nal * es::kCcSlotBytes;

  // ---- a. this lane's row: every wave loads the chunk's 64 rows and comes to the same ballot
  const int k = chunk * kCcChunkRows + lane;
  int off = 0, n = 0;
  bool cand = false;
  if (k < R) {
    const v4i row = rows[k];
    off = static_cast<int>(clamp(row[es::kNalOffset], 0, c.cap));
    n = static_cast<int>(clamp(row[es::kNalLength], 0, c.cap - off));
    cand = es::cc_nal_candidate(hevc, row[es::kNalType], row[es::kNalAu], m, n);
  }
  int flag = cand ? es::kCfCandidate | (n > es::kCcNalBytes ? es::kCfClipped : 0) : 0;

  // ---- b. the chunk's candidates go to the four waves in turn; a wave takes its own one by one
  const __amdgpu_buffer_rsrc_t rsrc = es_segment_rsrc(b, seg);
  uint8_t* raw = s_raw[wave];
  uint8_t* U = s_rbsp[wave];
  const unsigned long long all = __ballot(cand);
  const bool mine = cand && (__popcll(all & ((1ull << lane) - 1ull)) & (kCcWaves - 1)) == wave;
  unsigned long long todo = __ballot(mine);
  // this lane's 16 bytes of the wave's candidate `at`; the next candidate's load is issued in front
  // of the current one's LDS work, so its latency hides behind the unescape and the walk
  auto fetch = [&](int at, int& len) {
    const int c_off = __builtin_amdgcn_readfirstlane(__shfl(off, at));
    len = __builtin_amdgcn_readfirstlane(__shfl(n, at));
    return ps_copy_lane(rsrc, c_off, len, es::kCcNalBytes, lane);
  };
  int next_n = 0;
  v4u next = {0, 0, 0, 0};
  if (todo) next = fetch(__builtin_ctzll(todo), next_n);
  while (todo) {
    const int from = __builtin_ctzll(todo);
    todo &= todo - 1;
    const v4u mine = next;
    const int c_n = next_n;
    if (todo) next = fetch(__builtin_ctzll(todo), next_n);
    const int stored = c_n < es::kCcNalBytes ? c_n : es::kCcNalBytes;
    *reinterpret_cast<v4u*>(raw + lane * 16) = mine;
    cc_wave_sync();
    int u = 0;
    for (int jb = 0; jb < stored; jb += 64) {
      const int j = jb + lane;
      bool keep = false;
      uint8_t v = 0;
      if (j >= h && j < stored) {
        v = raw[j];
        keep = j < 2 || !es::is_emulation_prevention(raw[j - 2], raw[j - 1], v);
      }
      const unsigned long long mk = __ballot(keep);
      if (keep) U[u + __popcll(mk & ((1ull << lane) - 1ull))] = v;
      u += __popcll(mk);
    }
    cc_wave_sync();
    const uint8_t* up = U;
    const es::CcMatch hit = es::cc_find([up](int i) { return static_cast<int>(up[i]); }, u);
    if (hit.count >= 0) {
      const int size = 2 + 3 * hit.count;
      if (lane == from) flag |= es::kCfHit | (size << es::kCfSizeShift);
      if (lane < es::kCcSlotBytes / 16) {
        v4u q = {0, 0, 0, 0};
#pragma unroll
        for (int d = 0; d < 4; ++d) {
          uint32_t w = 0;
#pragma unroll
          for (int x = 0; x < 4; ++x) {
            const int i = lane * 16 + d * 4 + x;
            if (i < size) w |= static_cast<uint32_t>(U[hit.at + i]) << (8 * x);
          }
          q[d] = w;
        }
        const int64_t row_k = chunk * kCcChunkRows + from;
        *reinterpret_cast<v4u*>(hit_seg + row_k * es::kCcSlotBytes + lane * 16) = q;
      }
    }
    cc_wave_sync();  // raw and U are free for the next candidate
  }
  // a candidate's flag comes from the wave that walked it, every other row's from wave 0
  if (k < R && (mine || (!cand && wave == 0))) flag_seg[k] = flag;
}

__global__ __launch_bounds__(kCcThreads) void cc_pack_kernel(EsBatchView b, const uint8_t* __restrict__ enable,
                                                             const int32_t* __restrict__ flag_all,
                                                             const uint8_t* __restrict__ hit_all, int max_cc,
                                                             int32_t* __restrict__ samples_all,
                                                             int64_t* __restrict__ pts_all, uint8_t* __restrict__ bytes_all,
                                                             uint8_t* __restrict__ cc608_all,
                                                             int64_t* __restrict__ ccinfo_all) {
  __shared__ long long s_pts[es::kMaxCcLimit];
  __shared__ long long s_minmax[2];
  __shared__ int s_wave[kCcWaves];
  __shared__ int s_tot[5];  // candidates, clipped ones, triples, field 1 pairs, field 2 pairs
  const int seg = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63;
  const bool on = enable[seg] != 0;
  const auto c = es_segment(b, seg);
  const int R = on ? static_cast<int>(c.R) : 0;
  const v4i* rows = reinterpret_cast<const v4i*>(c.ix.nal);
  const int64_t* vp = es::pes_rows(c.sg).video;
  const int32_t* flag_seg = flag_all + static_cast<int64_t>(seg) * b.max_nal;
  const uint8_t* hit_seg = hit_all + static_cast<int64_t>(seg) * b.max_nal * es::kCcSlotBytes;
  int32_t* samples = samples_all + table_words(seg, max_cc, es::kCcRowWords);
  int64_t* pts_out = pts_all + static_cast<int64_t>(seg) * max_cc;
  uint8_t* bytes = bytes_all + static_cast<int64_t>(seg) * max_cc * es::kCcSlotBytes;
  uint8_t* cc608 = cc608_all + static_cast<int64_t>(seg) * max_cc * 2 * es::kCcFieldBytes;
  if (tid < 5) s_tot[tid] = 0;
  if (tid == 0) {
    s_minmax[0] = 0x7fffffffffffffffll;
    s_minmax[1] = -0x7fffffffffffffffll - 1;
  }
  __syncthreads();

  // ---- a. rank the hits in row order, a lane per row; the lane of a recorded hit writes its sample
  int carry = 0, n_cand = 0, n_clip = 0, n_tri = 0, n_f1 = 0, n_f2 = 0;
  for (int kb = 0; kb < R; kb += kCcThreads) {
    const int k = kb + tid;
    const int f = k < R ? flag_seg[k] : 0;
    const bool hit = (f & es::kCfHit) != 0;
    n_cand += (f & es::kCfCandidate) ? 1 : 0;
    n_clip += (f & es::kCfClipped) ? 1 : 0;
    const int inc = __popcll(__ballot(hit) & (~0ull >> (63 - lane)));  // hits up to this lane's
    const WgPrefix<int> p = wg_exclusive_prefix<kCcWaves>(inc, hit ? 1 : 0, s_wave);
    const int rank = carry + p.before;
    if (hit && rank < max_cc) {
      int size = (f >> es::kCfSizeShift) & 0xff;
      size = size < 2 ? 2 : size > 2 + 3 * es::kCcMaxTriples ? 2 + 3 * es::kCcMaxTriples : size;
      const int count = (size - 2) / 3;
      const int au = rows[k][es::kNalAu];
      const int64_t pts = es::pes_at(vp, clamp(au, 0, b.max_pes - 1), ts::kPesPts);
      const v4u* src = reinterpret_cast<const v4u*>(hit_seg + static_cast<int64_t>(k) * es::kCcSlotBytes);
      v4u* dst = reinterpret_cast<v4u*>(bytes + static_cast<int64_t>(rank) * es::kCcSlotBytes);
      uint32_t w[es::kCcSlotBytes / 4];
#pragma unroll
      for (int i = 0; i < es::kCcSlotBytes / 16; ++i) {
        const v4u v = src[i];
        dst[i] = v;
        w[4 * i] = v.x, w[4 * i + 1] = v.y, w[4 * i + 2] = v.z, w[4 * i + 3] = v.w;
      }
      uint16_t* f608 = reinterpret_cast<uint16_t*>(cc608 + static_cast<int64_t>(rank) * 2 * es::kCcFieldBytes);
      int p0 = 0, p1 = 0;
#pragma unroll
      for (int i = 0; i < 2 * es::kCcFieldBytes / 16; ++i) reinterpret_cast<v4u*>(f608)[i] = v4u{0, 0, 0, 0};
#pragma unroll
      for (int t = 0; t < es::kCcMaxTriples; ++t) {
        if (t < count) {
          const int i0 = 2 + 3 * t, i1 = 3 + 3 * t, i2 = 4 + 3 * t;
          const int fb = (w[i0 >> 2] >> (8 * (i0 & 3))) & 0xff;
          const int b1 = (w[i1 >> 2] >> (8 * (i1 & 3))) & 0xff;
          const int b2 = (w[i2 >> 2] >> (8 * (i2 & 3))) & 0xff;
          const int field = es::cc_608_field(fb, b1, b2);
          const uint16_t pair = static_cast<uint16_t>((b1 & 0x7f) | ((b2 & 0x7f) << 8));
          if (field == 0) f608[p0++] = pair;
          else if (field == 1) f608[es::kCcFieldBytes / 2 + p1++] = pair;
        }
      }
      int32_t* sr = samples + es::kCcRowWords * rank;  // kCrOrder is step b's
      sr[es::kCrNal] = k;
      sr[es::kCrAu] = au;
      sr[es::kCrSize] = size;
      sr[es::kCrCount] = count;
      sr[es::kCrField1Pairs] = p0;
      sr[es::kCrField2Pairs] = p1;
      sr[es::kCrFlags] = (w[0] & 0x40) ? es::kCcProcess : 0;
      pts_out[rank] = pts;
      s_pts[rank] = pts;
      __hip_atomic_fetch_min(&s_minmax[0], static_cast<long long>(pts), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      __hip_atomic_fetch_max(&s_minmax[1], static_cast<long long>(pts), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      n_tri += count;
      n_f1 += p0;
      n_f2 += p1;
    }
    carry += p.total;
    __syncthreads();  // s_wave is free again
  }
  if (n_cand) atomicAdd(&s_tot[0], n_cand);
  if (n_clip) atomicAdd(&s_tot[1], n_clip);
  if (n_tri) atomicAdd(&s_tot[2], n_tri);
  if (n_f1) atomicAdd(&s_tot[3], n_f1);
  if (n_f2) atomicAdd(&s_tot[4], n_f2);
  __syncthreads();
  const int n_rec = carry < max_cc ? carry : max_cc;

  // ---- b. presentation rank: a lane per recorded sample counts the samples in front of it
  for (int r = tid; r < n_rec; r += kCcThreads) {
    const long long p = s_pts[r];
    int order = 0;
    for (int q = 0; q < n_rec; ++q) {
      const long long pq = s_pts[q];
      order += (pq < p || (pq == p && q < r)) ? 1 : 0;
    }
    samples[es::kCcRowWords * r + es::kCrOrder] = order;
  }

  // ---- c. the rows beyond the recorded count, 16 bytes per store
  const v4i minus = {-1, -1, -1, -1};
  const v4u zero = {0, 0, 0, 0};
  for (int v = n_rec * 2 + tid; v < max_cc * 2; v += kCcThreads) reinterpret_cast<v4i*>(samples)[v] = minus;
  for (int v = n_rec + tid; v < max_cc; v += kCcThreads) pts_out[v] = -1;
  for (int v = n_rec * (es::kCcSlotBytes / 16) + tid; v < max_cc * (es::kCcSlotBytes / 16); v += kCcThreads)
    reinterpret_cast<v4u*>(bytes)[v] = zero;
  for (int v = n_rec * (es::kCcFieldBytes / 8) + tid; v < max_cc * (es::kCcFieldBytes / 8); v += kCcThreads)
    reinterpret_cast<v4u*>(cc608)[v] = zero;

  // ---- d. the info row
  if (tid == 0) {
    int64_t* ci = ccinfo_all + static_cast<int64_t>(seg) * es::kCcInfoWords;
    int64_t status = 0;
    if (on) {
      status = es::cc_status(c.sg, c.ix.sinfo);
      if (carry > max_cc) status |= es::kCcOverflow;
      if (s_tot[1]) status |= es::kCcSeiClipped;
    }
    ci[es::kCiStatus] = status;
    ci[es::kCiNumSei] = s_tot[0];
    ci[es::kCiNumSamples] = carry;
    ci[es::kCiNumTriples] = s_tot[2];
    ci[es::kCiField1Pairs] = s_tot[3];
    ci[es::kCiField2Pairs] = s_tot[4];
    ci[es::kCiFirstPts] = !on ? 0 : n_rec ? s_minmax[0] : -1;
    ci[es::kCiLastPts] = !on ? 0 : n_rec ? s_minmax[1] : -1;
  }
}

hipError_t launch_cc_extract(const CcExtractArgs& a) {
  const EsBatch& b = a.b;
  if (b.nseg <= 0) return hipSuccess;
  const EsBatchView view = es_batch_view(b);
  const es::CcScratch sc = es::cc_scratch(b.nseg, b.max_nal);
  int32_t* flag = a.scratch + sc.flag;
  uint8_t* hit = reinterpret_cast<uint8_t*>(a.scratch + sc.hit);
  const unsigned chunks = static_cast<unsigned>((b.max_nal + kCcChunkRows - 1) / kCcChunkRows);
  hipLaunchKernelGGL(cc_scan_kernel, dim3(chunks, b.nseg), dim3(kCcThreads), 0, b.stream, view, a.enable, flag, hit);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(cc_pack_kernel, dim3(b.nseg), dim3(kCcThreads), 0, b.stream, view, a.enable, flag, hit,
                     static_cast<int>(a.max_cc), a.t.samples, a.t.pts, a.t.bytes, a.t.cc608, a.t.info);
  return hipGetLastError();
}

}  // namespace dev
}  // namespace hlsp2p
