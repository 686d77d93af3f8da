// The moof boxes of remuxed segments (docs/FRAGMENT.md) — CDNA4 / gfx950.
//
// Input: what remux.hip leaves in HBM (rinfo, vsamples, asamples), the index's sinfo row for the
// audio sample rate (or, with a mpainfo row that has a config, that row's rate and frame:
// docs/MPEGAUDIO.md), and one fparams row per segment from the host (where the segment's region
// lies, the mfhd sequence number, the time base, the reference time, the anchor flag).  Output per
// segment, identical to the host implementation runtime/fragment.cpp fragment_segment:
//   out:   the video moof, right-aligned so that it ends where the video mdat starts (out_off),
//          and the audio moof, right-aligned so that it ends where the audio mdat starts
//          (out_off + A0): each moof and its mdat are one byte range
//   finfo: int64[seg][kFinfoWords]
// Nothing else of out is written: the rest of the headroom, the rest of the gap, both mdat boxes.
//
// One launch, one 256-thread workgroup per segment, no workgroup waits for another one:
//   - the asamples rows with offset >= 0 are counted by ballot and popcount, a wave total each
//     through LDS;
//   - a lane per vsamples row swaps duration, size, flags and cts to big-endian (v_perm) and
//     stores one aligned 16-byte trun entry: the moof ends at a 16-byte aligned address and the
//     entries are 16 bytes, so every entry is aligned;
//   - a lane per four audio trun entries, counted back from the aligned end, stores one 16-byte
//     vector; the ragged group at the head goes as dwords;
//   - 22 + 24 lanes write the dwords in front of the entries, one lane the finfo row.
// Every table read is bounded by max_pes / max_aframes, every write lies inside the headroom or
// the gap: the sample count is clamped to max_pes, the frame count cannot exceed max_aframes, and
// A0 is brought inside the region (es::frag_audio_box).  The time rules and the box words are
// shared/grammar.hpp (es::frag_times, es::moof_video_word, es::moof_audio_word), the same
// functions runtime/fragment.cpp calls.
#include "common.h"
#include "grammar.hpp"
#include "launch.h"

namespace hlsp2p {
namespace dev {

constexpr int kFrThreads = 256;
constexpr int kFrWaves = kFrThreads / 64;
constexpr int kFrAudioLane0 = 64;  // the first lane of the audio header's writers: a wave of its own

__device__ __forceinline__ uint32_t fr_be32(uint32_t x) { return __builtin_amdgcn_perm(0u, x, 0x00010203u); }
__device__ __forceinline__ uint32_t fr_be32(int32_t x) { return fr_be32(static_cast<uint32_t>(x)); }

__global__ __launch_bounds__(kFrThreads) void fragment_moof_kernel(
    const int64_t* __restrict__ rinfo, const int32_t* __restrict__ vs_all, const int32_t* __restrict__ as_all,
    const int64_t* __restrict__ sinfo, const int64_t* __restrict__ fparams, int64_t max_pes, int64_t max_aframes,
    int64_t headroom, int64_t audio_gap, uint8_t* __restrict__ out, int64_t out_numel, int64_t* __restrict__ finfo,
    const int64_t* __restrict__ mpainfo) {
  __shared__ int s_cnt[kFrWaves];
  const int seg = blockIdx.x;
  const int tid = threadIdx.x;
  const int64_t* fp = fparams + static_cast<int64_t>(seg) * es::kFparamWords;
  const int64_t oo = fp[es::kFpOutOff], region = fp[es::kFpRegion];
  // workgroup-uniform: a row that does not lie inside out writes nothing
  if (oo < headroom || (oo & 15) != 0 || region < audio_gap + 32 || oo > out_numel || region > out_numel - oo) return;
  const int64_t* ri = rinfo + static_cast<int64_t>(seg) * es::kRinfoWords;
  const int32_t* vs = vs_all + table_words(seg, max_pes, es::kVsampleWords);
  const int32_t* as = as_all + table_words(seg, max_aframes, es::kAsampleWords);
  const int64_t m = clamp(ri[es::kNumVsamples], 0, max_pes);
  const int64_t A0 = es::frag_audio_box(ri[es::kAudioBoxOffset], region, audio_gap);

  // ---- the recorded frames: rows with offset >= 0
  int wave_cnt = 0;
  for (int64_t fb = 0; fb < max_aframes; fb += kFrThreads) {  // workgroup-uniform trip count
    const int64_t f = fb + tid;
    const bool filled = f < max_aframes && as[es::kAsampleWords * f + es::kAsOffset] >= 0;
    wave_cnt += __popcll(__ballot(filled));
  }
  if ((tid & 63) == 0) s_cnt[tid >> 6] = wave_cnt;
  __syncthreads();
  int64_t n = 0;
#pragma unroll
  for (int w = 0; w < kFrWaves; ++w) n += s_cnt[w];

  const es::FragAudio fa = es::frag_audio(sinfo[static_cast<int64_t>(seg) * es::kSinfoWords + es::kAudioSampleRate],
                                          mpainfo ? mpainfo + static_cast<int64_t>(seg) * es::kMpainfoWords : nullptr);
  const es::FragTimes ft = es::frag_times(m, ri[es::kVideoBaseDts], ri[es::kAudioBasePts], fa.rate,
                                          fp[es::kFpTimeBase], fp[es::kFpTimeRef], fp[es::kFpAnchor] != 0);
  const uint32_t seq = static_cast<uint32_t>(fp[es::kFpSequence]);
  const int64_t vbytes = es::moof_video_bytes(m), abytes = es::moof_audio_bytes(n);
  uint8_t* vend = out + oo;   // 16-byte aligned: out is, and oo
  uint8_t* aend = vend + A0;  // A0 is a multiple of 16

  // ---- video trun entries: duration, size, flags, cts
  for (int64_t a = tid; a < m; a += kFrThreads) {
    const int32_t* row = vs + a * es::kVsampleWords;
    const v4u e = {fr_be32(row[es::kVsDuration]), fr_be32(row[es::kVsSize]), fr_be32(row[es::kVsFlags]),
                   fr_be32(row[es::kVsCts])};
    *reinterpret_cast<v4u*>(vend - es::kMoofVideoEntry * (m - a)) = e;
  }
  // ---- audio trun entries: the sizes of the first n rows, four to a vector from the end backwards
  const int64_t groups = n >> 2, ragged = n & 3;
  for (int64_t g = tid; g < groups; g += kFrThreads) {
    const int32_t* row = as + es::kAsampleWords * (n - 4 * (g + 1)) + es::kAsSize;
    const v4u e = {fr_be32(row[0]), fr_be32(row[es::kAsampleWords]), fr_be32(row[2 * es::kAsampleWords]),
                   fr_be32(row[3 * es::kAsampleWords])};
    *reinterpret_cast<v4u*>(aend - 16 * (g + 1)) = e;
  }
  if (tid < ragged)
    *reinterpret_cast<uint32_t*>(aend - es::kMoofAudioEntry * (n - tid)) = fr_be32(as[es::kAsampleWords * tid + es::kAsSize]);

  // ---- the dwords in front of the entries, and the finfo row
  if (tid < es::kMoofVideoHead / 4) {
    *reinterpret_cast<uint32_t*>(vend - vbytes + 4 * tid) =
        fr_be32(es::moof_video_word(tid, static_cast<uint32_t>(m), seq, static_cast<uint64_t>(ft.video_tfdt)));
  } else if (tid >= kFrAudioLane0 && tid < kFrAudioLane0 + es::kMoofAudioHead / 4) {
    const int i = tid - kFrAudioLane0;
    *reinterpret_cast<uint32_t*>(aend - abytes + 4 * i) =
        fr_be32(es::moof_audio_word(i, static_cast<uint32_t>(n), seq, static_cast<uint64_t>(ft.audio_tfdt), fa.duration));
  } else if (tid == 2 * kFrAudioLane0) {
    int64_t* fi = finfo + static_cast<int64_t>(seg) * es::kFinfoWords;
    fi[es::kFStatus] = ft.status;
    fi[es::kFVideoMoofBytes] = vbytes;
    fi[es::kFAudioMoofBytes] = abytes;
    fi[es::kFVideoTfdt] = ft.video_tfdt;
    fi[es::kFAudioTfdt] = ft.audio_tfdt;
    fi[es::kFTimeBase] = ft.base;
    fi[es::kFNumAsamples] = n;
    fi[es::kFSpare] = 0;
  }
}

hipError_t launch_fragment_moof(const FragmentArgs& a) {
  if (a.nseg <= 0) return hipSuccess;
  hipLaunchKernelGGL(fragment_moof_kernel, dim3(a.nseg), dim3(kFrThreads), 0, a.stream, a.rinfo, a.vsamples, a.asamples,
                     a.sinfo, a.fparams, a.max_pes, a.max_aframes, a.headroom, a.audio_gap, a.out, a.out_numel, a.finfo,
                     a.mpainfo);
  return hipGetLastError();
}

}  // namespace dev
}  // namespace hlsp2p
