// HLS SAMPLE-AES decryption of demuxed and indexed segments in place (docs/SAMPLEAES.md) — CDNA4 /
// gfx950.
//
// Input: what ts_demux.hip and es_index.hip leave in HBM, one key schedule and one IV per segment.
// Output, identical to the host implementation runtime/sampleaes.cpp sample_decrypt_segment:
//   es:     every protected H.264 slice NAL unescaped where it lies, its cipher blocks decrypted,
//           zeros behind it; the cipher blocks of every counted ADTS frame decrypted
//   nal:    the length column of a protected row becomes the unescaped length
//   sainfo: int64[seg][kSaWords]
//
// Two launches on the caller's stream, no host round trip and no scratch (the host caps, max_pes
// and max_nal size the grid and bound every access):
//   1. sample_aes_plan_kernel — a lane per segment: the status bits and zero counts of its sainfo row.
//   2. sample_aes_kernel      — 256-thread workgroups on a grid of min(max_pes, kSaGridUnits) x
//                               segments x 2: workgroup x takes the access units (z = 0) or audio
//                               PES (z = 1) x, x + gridDim.x, .. of its segment, so a usual
//                               segment has one per workgroup; workgroups past the real counts, of
//                               segments that did not ask and of other codecs exit before the
//                               first barrier.
//      video: the workgroup walks the NAL rows of its access unit.  A candidate longer than 48 raw
//             bytes is walked twice in rounds of kSaRound raw bytes, 16 per lane (common.h
//             load16_unaligned) through the segment's buffer resource (es_dev.h es_segment_rsrc:
//             it ends with the ES tensor): first only counted (the NAL sits in L2 for
//             the second walk), then, if it is protected, compacted into an LDS staging area
//             (emulation-prevention flags from the two raw predecessors, popcount prefix in the
//             wave by DPP, four wave totals through LDS (common.h wg_exclusive_prefix), a carry
//             across rounds), a lane per
//             cipher block decrypts there, and the staged bytes go back to global in 16-byte
//             vectors.  Compaction only moves bytes towards lower addresses inside the
//             workgroup's own NAL, and a round stores only behind a barrier that follows its loads.
//      audio: the workgroup walks the counted frames of its PES; a lane per cipher block, the
//             blocks of a frame in descending rounds of 256.
// No workgroup waits for another one: the order comes from the launches alone.  Counts reach
// sainfo by integer atomics.  All stores are vector stores.
// The three hazards of working in place are named where they are handled (hazard 1, 2, 3).
// The candidate / protected / cipher-block rules, the emulation-prevention predicate, the ADTS
// frame rule and the segment view are shared/grammar.hpp (namespace es), the same functions
// runtime/sampleaes.cpp calls.
#include "aes_small_dev.h"
#include "es_dev.h"

namespace hlsp2p {
namespace dev {

constexpr int kSaThreads = 256;
constexpr int kSaWaves = kSaThreads / 64;
// staging: the alignment shift (< 16), a carried unfinished block (< 16) and one round
constexpr int kSaStage = es::kSaRound + 32;
// grid.x: with max_pes rows per segment (512 by default) a workgroup per row would launch tens of
// thousands of workgroups that exit at once; beyond this many units a workgroup takes several
constexpr int kSaGridUnits = 128;
static_assert(kSaThreads * 16 == es::kSaRound, "a lane per 16 raw bytes of a round");
static_assert((es::kSaRound + 16) / es::kSaBlockStride + 2 <= kSaThreads, "a lane per cipher block of a flush");
static_assert(es::kAesBlock == 16 && es::kSaWords <= 8, "16-byte blocks, a short sainfo row");
int sample_aes_round_bytes() { return es::kSaRound; }

using SaBatchView = EsBatchViewOf<int32_t, const int64_t>;  // the length column of nal is rewritten

// load16_unaligned's 16 bytes as the AES helpers take them
__device__ __forceinline__ uint4 sa_u4(v4u q) { return uint4{q.x, q.y, q.z, q.w}; }
__device__ __forceinline__ uint32_t sa_word(const uint4& q, int d) { return d == 0 ? q.x : d == 1 ? q.y : d == 2 ? q.z : q.w; }
__device__ __forceinline__ int sa_byte(const uint4& q, int j) { return (sa_word(q, j >> 2) >> (8 * (j & 3))) & 0xff; }
__device__ __forceinline__ uint4 sa_xor(const uint4& a, const uint4& b) { return uint4{a.x ^ b.x, a.y ^ b.y, a.z ^ b.z, a.w ^ b.w}; }
// 16 bytes of LDS at any alignment
__device__ __forceinline__ uint4 sa_lds16(const uint8_t* p) {
  uint32_t w[4];
#pragma unroll
  for (int d = 0; d < 4; ++d)
    w[d] = p[4 * d] | (static_cast<uint32_t>(p[4 * d + 1]) << 8) | (static_cast<uint32_t>(p[4 * d + 2]) << 16) |
           (static_cast<uint32_t>(p[4 * d + 3]) << 24);
  return uint4{w[0], w[1], w[2], w[3]};
}
__device__ __forceinline__ void sa_put16(uint8_t* p, const uint4& q) {
#pragma unroll
  for (int j = 0; j < 16; ++j) p[j] = static_cast<uint8_t>(sa_byte(q, j));
}

// ---------------------------------------------------------------- 1. plan
// Both kernels take the batch as separate parameters and make the view themselves: see
// sample_aes_kernel.  This one reads no index table but sinfo.
__global__ __launch_bounds__(kSaThreads) void sample_aes_plan_kernel(
    const uint8_t* __restrict__ es, const int64_t* __restrict__ es_off, const int64_t* __restrict__ cap,
    const int64_t* __restrict__ info, const int64_t* __restrict__ pes, int64_t max_pes, int64_t max_nal,
    const int64_t* __restrict__ sinfo, const uint8_t* __restrict__ enable, int64_t* __restrict__ sainfo, int nseg) {
  const int seg = blockIdx.x * kSaThreads + threadIdx.x;
  if (seg >= nseg) return;
  int64_t status = 0;
  if (enable[seg]) {
    const EsBatchView b{es, 0, es_off, cap, info, pes, max_pes, max_nal, {nullptr, nullptr, nullptr, sinfo}};
    status = es::sample_status(es_segment_clamped(b, seg), sinfo + static_cast<int64_t>(seg) * es::kSinfoWords);
  }
  int64_t* row = sainfo + static_cast<int64_t>(seg) * es::kSaWords;
#pragma unroll
  for (int w = 0; w < es::kSaWords; ++w) row[w] = w == es::kSaStatus ? status : 0;
}

// ---------------------------------------------------------------- 2. decrypt
// What a round's scan leaves in a lane: its 16 raw bytes, which of them stay (bit j: byte j), how
// many unescaped bytes lie in front of its first one inside the round, and the round's total.
struct SaScan {
  uint4 q;
  uint32_t keep;
  int before, total;
};

// Round t of the NAL at segment offset nal_off with n raw bytes, called by the whole workgroup:
// 16 raw bytes per lane into s_raw[16 + 16 tid ..], the emulation-prevention flags from each
// byte's two raw predecessors, and the prefix of the kept bytes.  s_raw[14..15] are the two raw
// bytes in front of the round, left there by the round before (hazard 1).
__device__ __forceinline__ SaScan sa_scan_round(__amdgpu_buffer_rsrc_t rsrc, int nal_off, int n, int t, uint8_t* s_raw,
                                                int* s_wave) {
  const int tid = threadIdx.x;
  const int64_t p = static_cast<int64_t>(t) * es::kSaRound + tid * 16;  // this lane's first raw byte
  const int nv = static_cast<int>(clamp(n - p, 0, 16));
  SaScan r = {uint4{0, 0, 0, 0}, 0, 0, 0};
  if (nv > 0) r.q = sa_u4(load16_unaligned(rsrc, nal_off + static_cast<int>(p)));
  *reinterpret_cast<uint4*>(s_raw + 16 + tid * 16) = r.q;
  // every load of the round has returned (its data is in LDS) before any thread goes on to store
  __syncthreads();
  int p2 = s_raw[14 + tid * 16], p1 = s_raw[15 + tid * 16];
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    const int b = sa_byte(r.q, j);
    if (j < nv && !(p + j >= 2 && es::is_emulation_prevention(p2, p1, b))) r.keep |= 1u << j;
    p2 = p1;
    p1 = b;
  }
  const int cnt = __popc(r.keep);
  const WgPrefix<int> pre = wg_exclusive_prefix<kSaWaves>(static_cast<int>(wave_scan_dpp(cnt)), cnt, s_wave);
  r.before = pre.before;
  r.total = pre.total;
  // hazard 1: the round's last two raw bytes are the next round's predecessors, and this round's
  // own write-back may overwrite them in global memory: they stay in LDS.  Every thread has read
  // its predecessors in front of the barrier above.
  if (tid == kSaThreads - 1) {
    s_raw[14] = static_cast<uint8_t>(sa_byte(r.q, 14));
    s_raw[15] = static_cast<uint8_t>(sa_byte(r.q, 15));
  }
  return r;
}

// The batch arrives as separate parameters here and becomes a view in the kernel: only a kernel
// argument carries readonly and noalias, which keep the uniform loads of the unit loops scalar
// while the kernel stores to es and nal.  es is read and written, nal_all written: no qualifier.
__global__ __launch_bounds__(kSaThreads) void sample_aes_kernel(
    uint8_t* es, int64_t es_numel, const int64_t* __restrict__ es_off, const int64_t* __restrict__ cap,
    const int64_t* __restrict__ info, const int64_t* __restrict__ pes, int64_t max_pes, int64_t max_nal,
    int32_t* nal_all, const int32_t* __restrict__ au_all, const int32_t* __restrict__ af_all,
    const int64_t* __restrict__ sinfo, const uint32_t* __restrict__ rk_all, const uint8_t* __restrict__ iv_all,
    const uint8_t* __restrict__ enable, const uint32_t* __restrict__ tdl, const uint8_t* __restrict__ isb,
    int64_t* sainfo_all) {
  __shared__ AesSmallLds s_aes;
  __shared__ __attribute__((aligned(16))) uint8_t s_raw[16 + es::kSaRound];
  __shared__ __attribute__((aligned(16))) uint8_t s_stage[kSaStage];
  __shared__ uint4 s_chain;
  __shared__ int s_wave[kSaWaves];
  __shared__ int s_frame[2];
  const int seg = blockIdx.y;
  const bool is_audio = blockIdx.z != 0;
  const int tid = threadIdx.x;
  if (!enable[seg]) return;
  const SaBatchView b{es, es_numel, es_off, cap, info, pes, max_pes, max_nal,
                      {nal_all, const_cast<int32_t*>(au_all), const_cast<int32_t*>(af_all), sinfo}};
  const auto sv = es_segment(b, seg);
  const es::Segment& sg = sv.sg;
  const es::IndexTables<int32_t, const int64_t>& ix = sv.ix;
  const int cap_es = sv.cap;
  uint8_t* E = es + b.es_off[seg];  // es is b.es, writable; 16-byte aligned: the tensor is, and so is every offset
  const __amdgpu_buffer_rsrc_t rsrc = es_segment_rsrc(b, seg);
  const uint4 iv = *reinterpret_cast<const uint4*>(iv_all + static_cast<int64_t>(seg) * es::kAesBlock);
  const uint32_t* rk = rk_all + static_cast<int64_t>(seg) * es::kAesRoundKeyWords;
  unsigned long long* sainfo = reinterpret_cast<unsigned long long*>(sainfo_all + static_cast<int64_t>(seg) * es::kSaWords);

  if (!is_audio) {
    // ------------------------------------------------------------ video: one access unit
    if (sg.info[ts::kVideoType] != ts::kAvc) return;
    const int64_t R = sv.R, m = sv.m;
    if (static_cast<int64_t>(blockIdx.x) >= m) return;
    aes_small_fill(s_aes, tdl, isb, rk, tid);
    __syncthreads();
    int64_t n_prot = 0, n_removed = 0, n_blocks = 0;
    for (int unit = blockIdx.x; unit < m; unit += gridDim.x) {
      const int32_t* aurow = ix.au + es::kAuWords * static_cast<int64_t>(unit);
      const int64_t first = clamp(aurow[es::kAuFirstNal], 0, R);
      const int64_t last = clamp(first + aurow[es::kAuNalCount], first, R);
      for (int64_t k = first; k < last; ++k) {
        // a row belongs to the one access unit it names: no two workgroups take the same row
        int32_t* row = ix.nal + es::kNalWords * k;
        const int nal_off = static_cast<int>(clamp(row[es::kNalOffset], 0, cap_es));
        const int n = static_cast<int>(clamp(row[es::kNalLength], 0, cap_es - nal_off));
        if (row[es::kNalAu] != unit || !es::sample_nal_candidate(row[es::kNalType], unit, m, n)) continue;
        if (!es::sample_nal_protected(n)) continue;  // u <= n
        const int rounds = (n + es::kSaRound - 1) / es::kSaRound;

        // ---- first walk: the unescaped length
        int u = 0;
        for (int t = 0; t < rounds; ++t) u += sa_scan_round(rsrc, nal_off, n, t, s_raw, s_wave).total;
        if (!es::sample_nal_protected(u)) continue;

        // ---- second walk: compact, decrypt, store.  The staging area holds the unescaped bytes
        // [S0, E1); byte p of them sits at s_stage[p - S0 + sh] with sh = (nal_off + S0) & 15, so a
        // 16-byte chunk of the area is a 16-byte aligned chunk of global memory.
        int S0 = 0, E1 = 0, sh = nal_off & 15;
        for (int t = 0; t < rounds; ++t) {
          const SaScan sc = sa_scan_round(rsrc, nal_off, n, t, s_raw, s_wave);
          int pos = E1 + sc.before - S0 + sh;
  #pragma unroll
          for (int j = 0; j < 16; ++j)
            if (sc.keep & (1u << j)) s_stage[pos++] = static_cast<uint8_t>(sa_byte(sc.q, j));
          E1 += sc.total;
          __syncthreads();
          // hazard 3: a cipher block may straddle the round's edge in the unescaped domain.  Bytes
          // from the start of an unfinished block on stay in the staging area for the next round.
          int F = E1;
          if (t + 1 < rounds && E1 > es::kSaClearLead) {
            const int c = static_cast<int>(es::sample_block_at((E1 - es::kSaClearLead) / es::kSaBlockStride));
            if (E1 < c + es::kAesBlock) F = c;
          }
          // the cipher blocks that lie in [S0, F): a lane each
          const int j_lo = S0 <= es::kSaClearLead ? 0 : (S0 - es::kSaClearLead + es::kSaBlockStride - 1) / es::kSaBlockStride;
          const int limit = F < u - 1 ? F : u - 1;  // a block must end at or before F and strictly before u
          const int j_hi = limit >= es::kSaClearLead + es::kAesBlock
                               ? (limit - es::kSaClearLead - es::kAesBlock) / es::kSaBlockStride + 1 : 0;
          const int nblk = j_hi > j_lo ? j_hi - j_lo : 0;
          const bool mine = tid < nblk;
          const int at = mine ? static_cast<int>(es::sample_block_at(j_lo + tid)) - S0 + sh : 0;
          uint4 c4 = {0, 0, 0, 0}, p4 = {0, 0, 0, 0};
          if (mine) {
            // hazard 2: C_{j-1} is overwritten by P_{j-1}.  Every ciphertext of the flush is read in
            // front of the barrier below and every plaintext stored behind it; the last ciphertext
            // of a flush stays in s_chain for the first block of the next one.
            c4 = sa_lds16(s_stage + at);
            const uint4 chain = j_lo + tid == 0 ? iv : tid == 0 ? s_chain : sa_lds16(s_stage + at - es::kSaBlockStride);
            p4 = sa_xor(aes_small_decrypt(s_aes, c4), chain);
          }
          __syncthreads();
          if (mine) {
            sa_put16(s_stage + at, p4);
            if (tid == nblk - 1) s_chain = c4;
          }
          n_blocks += nblk;
          __syncthreads();
          // [S0, F) back to global: the loads of this round are complete, and no later round reads
          // below its own first raw byte, which is not below F
          const int gbase = nal_off + S0 - sh, end = sh + F - S0;
          for (int c = tid * 16; c < end; c += kSaThreads * 16) {
            if (c >= sh && c + 16 <= end) {
              *reinterpret_cast<uint4*>(E + gbase + c) = *reinterpret_cast<const uint4*>(s_stage + c);
            } else {
              const int lo = c > sh ? c : sh, hi = c + 16 < end ? c + 16 : end;
              for (int i = lo; i < hi; ++i) E[gbase + i] = s_stage[i];
            }
          }
          // the unfinished block moves to the front of the staging area
          const int keep_n = E1 - F, sh_next = (nal_off + F) & 15;
          uint8_t moved = 0;
          if (tid < keep_n) moved = s_stage[F - S0 + sh + tid];
          __syncthreads();
          if (tid < keep_n) s_stage[sh_next + tid] = moved;
          S0 = F;
          sh = sh_next;
        }
        // zeros behind the unescaped NAL: valid Annex-B trailing zeros
        for (int i = u + tid; i < n; i += kSaThreads) E[nal_off + i] = 0;
        if (tid == 0) row[es::kNalLength] = u;
        n_prot += 1;
        n_removed += n - u;
      }
    }
    if (tid == 0 && n_prot > 0) {
      atomicAdd(sainfo + es::kSaProtectedNals, static_cast<unsigned long long>(n_prot));
      atomicAdd(sainfo + es::kSaRemovedBytes, static_cast<unsigned long long>(n_removed));
      atomicAdd(sainfo + es::kSaVideoBlocks, static_cast<unsigned long long>(n_blocks));
    }
    return;
  }

  // -------------------------------------------------------------- audio: one PES
  const es::AudioSpan audio = es::audio_span(sg);
  if (static_cast<int64_t>(blockIdx.x) >= audio.n_adts) return;
  aes_small_fill(s_aes, tdl, isb, rk, tid);
  __syncthreads();
  const uint8_t* A = E + audio.off;
  int64_t n_frames = 0, n_blocks = 0;
  for (int unit = blockIdx.x; unit < audio.n_adts; unit += gridDim.x) {
    const es::ByteRange range = es::audio_pes_range(es::pes_rows(sg).audio, unit, audio);
    const int64_t want = ix.aframes[es::kApesWords * static_cast<int64_t>(unit) + es::kApesFrames];
    int64_t q = range.start;
    for (int64_t j = 0; j < want; ++j) {
      // one thread reads the header, so the whole workgroup takes one decision on any bytes
      if (tid == 0) {
        const es::AdtsFrame f = es::adts_frame_at(A, q, range.end);
        s_frame[0] = f.len;
        s_frame[1] = f.hdr;
      }
      __syncthreads();
      const es::AdtsFrame f = {s_frame[0], s_frame[1]};
      __syncthreads();
      if (f.len == 0) break;
      const int nb = static_cast<int>(es::sample_audio_blocks(f));
      const int base = static_cast<int>(audio.off + q) + f.hdr + es::kSaAudioLead;  // inside the frame, below cap
      // hazard 2: C_{i-1} is overwritten by P_{i-1}.  Rounds of 256 blocks run from the frame's end
      // to its start, so a round's first block finds its predecessor still encrypted, and inside a
      // round every ciphertext is read in front of the barrier and every plaintext stored behind it.
      for (int ib = nb > 0 ? (nb - 1) / kSaThreads * kSaThreads : -1; ib >= 0; ib -= kSaThreads) {
        const int i = ib + tid;
        const bool mine = i < nb;
        uint4 p4 = {0, 0, 0, 0};
        if (mine) {
          const uint4 c4 = sa_u4(load16_unaligned(rsrc, base + es::kAesBlock * i));
          const uint4 chain = i == 0 ? iv : sa_u4(load16_unaligned(rsrc, base + es::kAesBlock * (i - 1)));
          p4 = sa_xor(aes_small_decrypt(s_aes, c4), chain);  // consumes the loads: they have returned
        }
        __syncthreads();
        if (mine) {
          uint8_t* dst = E + base + es::kAesBlock * i;
          if ((base & 3) == 0) {
            uint32_t* d32 = reinterpret_cast<uint32_t*>(dst);
            d32[0] = p4.x;
            d32[1] = p4.y;
            d32[2] = p4.z;
            d32[3] = p4.w;
          } else {
            sa_put16(dst, p4);
          }
        }
      }
      if (nb > 0) {
        n_frames += 1;
        n_blocks += nb;
      }
      q += f.len;
    }
  }
  if (tid == 0 && n_frames > 0) {
    atomicAdd(sainfo + es::kSaAudioFrames, static_cast<unsigned long long>(n_frames));
    atomicAdd(sainfo + es::kSaAudioBlocks, static_cast<unsigned long long>(n_blocks));
  }
}

hipError_t launch_sample_aes(const SampleAesArgs& a) {
  const EsBatch& b = a.b;
  if (b.nseg <= 0) return hipSuccess;
  hipLaunchKernelGGL(sample_aes_plan_kernel, dim3((b.nseg + kSaThreads - 1) / kSaThreads), dim3(kSaThreads), 0, b.stream,
                     b.es, b.es_off, b.cap, b.info, b.pes, b.max_pes, b.max_nal, b.ix.sinfo, a.enable, a.sainfo, b.nseg);
  const unsigned units = static_cast<unsigned>(b.max_pes < kSaGridUnits ? b.max_pes : kSaGridUnits);
  hipLaunchKernelGGL(sample_aes_kernel, dim3(units, b.nseg, 2), dim3(kSaThreads), 0, b.stream,
                     a.es, b.es_numel, b.es_off, b.cap, b.info, b.pes, b.max_pes, b.max_nal, b.ix.nal, b.ix.au,
                     b.ix.aframes, b.ix.sinfo, a.round_keys, a.iv, a.enable, a.td, a.isb, a.sainfo);
  return hipGetLastError();
}

}  // namespace dev
}  // namespace hlsp2p
