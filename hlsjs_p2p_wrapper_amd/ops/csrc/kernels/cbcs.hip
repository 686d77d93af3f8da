// cbcs (ISO/IEC 23001-7, HLS SAMPLE-AES on fragmented MP4) decryption of a demuxed batch into a
// copy (docs/CBCS.md) — CDNA4 / gfx950.
//
// Input: the segments where mp4_demux.hip read them, only read; its minfo / msamples / runs / info
// / pes; per segment two protection rows, two constant IVs, a fallback IV, a key schedule; and a
// destination that already holds a copy of every enabled segment.
// Output, identical to the host implementation runtime/cbcs.cpp cbcs_segment:
//   dst:    every cipher block of every recorded range decrypted, nothing else touched
//   ranges: int32[seg][max_range][kRangeWords]      cinfo: int64[seg][kCbInfoWords]
//
// Two launches on the caller's stream, ordered by the stream alone; no workgroup waits for another:
//   1. cbcs_plan_kernel — one 256-thread workgroup per segment.  Lane 0 walks the top level; a
//      lane per moof walks its trafs and the entries of their senc boxes (a latency chain over the
//      few KB the demux just read) and leaves each recorded sample's entry in scratch; the lanes
//      of the samples leave their runs' byte spans in LDS and a lane per run tests its span
//      against the runs in front of it (a run of a damaged file that shares bytes with an earlier
//      one is left encrypted, so no two chains ever write one byte); then, in rounds of 256
//      samples with a carry, a lane per sample counts its ranges and cipher blocks, two 64-bit
//      workgroup scans rank them, and the lane walks its subsamples again to write its rows.
//   2. cbcs_blocks_kernel — a lane per cipher block: tiles of 256 consecutive block ranks of one
//      segment on a grid of min(tiles, kCbGridTiles) x segments.  A workgroup narrows the ranges
//      its tile touches into LDS by a binary search at the tile's two ends; a lane finds its range
//      there, loads its block and the block in front (or the IV) from the SOURCE through a buffer
//      resource that ends with the segment, and stores the plaintext into the copy.  The source
//      is never written, so no chain reads a block that anyone has overwritten: no barrier
//      orders two blocks, no state is carried.
// Segments that did not ask, segments without a protected track and workgroups past a segment's
// block count exit before their first barrier.  All stores are vector stores.
// The senc, subsample, pattern and overlap rules are shared/grammar.hpp (namespace mp4), the same
// functions runtime/cbcs.cpp calls.
#include "aes_small_dev.h"
#include "launch.h"
#include "mp4_dev.h"

namespace hlsp2p {
namespace dev {

constexpr int kCbThreads = 256;
constexpr int kCbWaves = kCbThreads / 64;
// grid.x of the decrypt: the host knows only cap / 16, an upper bound of a segment's cipher blocks;
// beyond this many tiles a workgroup takes several
constexpr int kCbGridTiles = 64;
static_assert(mp4::kCbTileBlocks == kCbThreads, "a lane per cipher block of a tile");
static_assert(mp4::kMaxBoxRows == kCbThreads, "a lane per moof or run row in one round");
static_assert(mp4::kRangeWords == 4 && mp4::kAuxWords == 4 && mp4::kCbInfoWords % 2 == 0, "16-byte rows");

__device__ __forceinline__ int cbcs_segment_bytes(const CbcsArgs& a, int seg) {
  return static_cast<int>(clamp(a.info[static_cast<int64_t>(seg) * ts::kInfoWords + ts::kVideoBytes], 0,
                                clamp(a.cap[seg], 0, 0x7fffffff)));
}
__device__ __forceinline__ const int64_t* cbcs_pes(const CbcsArgs& a, int seg, int t) {
  return a.pes + ts::pes_words(seg, a.max_pes) + table_words(t, a.max_pes, ts::kPesWords);
}
__device__ __forceinline__ const v4i* cbcs_msamples(const CbcsArgs& a, int seg, int t) {
  return reinterpret_cast<const v4i*>(a.msamples + table_words(seg, mp4::kTracks * a.max_pes, mp4::kMsampleWords) +
                                      table_words(t, a.max_pes, mp4::kMsampleWords));
}
__device__ __forceinline__ v4i* cbcs_aux(const CbcsArgs& a, int seg, int t) {
  return reinterpret_cast<v4i*>(a.scratch) + (static_cast<int64_t>(seg) * mp4::kTracks + t) * a.max_pes;
}

// ---------------------------------------------------------------- 1. plan
__global__ __launch_bounds__(kCbThreads) void cbcs_plan_kernel(CbcsArgs a) {
  __shared__ long long s_wave0[kCbWaves], s_wave1[kCbWaves];
  __shared__ unsigned long long s_blocks[mp4::kTracks];
  __shared__ int s_moof_p[mp4::kMaxBoxRows], s_moof_hdr[mp4::kMaxBoxRows], s_moof_size[mp4::kMaxBoxRows];
  __shared__ int s_lo[mp4::kMaxBoxRows], s_hi[mp4::kMaxBoxRows], s_shadow[mp4::kMaxBoxRows];
  __shared__ int s_nm, s_status, s_nsenc, s_samples[mp4::kTracks];
  const int seg = blockIdx.x, tid = threadIdx.x;
  const int64_t max_range = a.max_range, max_pes = a.max_pes;
  v4i* rows = reinterpret_cast<v4i*>(a.ranges + table_words(seg, max_range, mp4::kRangeWords));
  v2l* ci = reinterpret_cast<v2l*>(a.cinfo + static_cast<int64_t>(seg) * mp4::kCbInfoWords);
  const int64_t* prot = a.prot + static_cast<int64_t>(seg) * mp4::kTracks * mp4::kProtWords;
  const int64_t* mi = a.minfo + static_cast<int64_t>(seg) * mp4::kMinfoWords;
  const bool on = a.enable[seg] != 0;
  const bool prot_on[mp4::kTracks] = {on && prot[mp4::kPrProtected] == 1,
                                      on && prot[mp4::kProtWords + mp4::kPrProtected] == 1};
  const int64_t damaged = on && (mi[mp4::kMStatus] & mp4::kCbDamagedMask) ? mp4::kCbDemuxDamaged : 0;
  if (!prot_on[0] && !prot_on[1]) {  // before the first barrier
    for (int64_t i = tid; i < max_range; i += kCbThreads) rows[i] = v4i{-1, -1, -1, -1};
    if (tid < mp4::kCbInfoWords / 2) ci[tid] = v2l{tid == 0 ? damaged : 0, 0};
    return;
  }
  const int64_t rec[mp4::kTracks] = {
      prot_on[0] ? clamp(mi[mp4::kMTrack0 + mp4::kMtNumSamples], 0, max_pes) : 0,
      prot_on[1] ? clamp(mi[mp4::kMTrack0 + mp4::kMTrackWords + mp4::kMtNumSamples], 0, max_pes) : 0};
  const int nr = static_cast<int>(clamp(mi[mp4::kMNumRun], 0, a.max_run));
  const int64_t* runs = a.runs + table_words(seg, a.max_run, mp4::kRunWords);
  const int n = cbcs_segment_bytes(a, seg);
  SegReader rd = mp4_reader(a.src, a.src_numel, a.src_off[seg], n);
  const int iv_size[mp4::kTracks] = {mp4::iv_bytes(prot[mp4::kPrIvSize]),
                                     mp4::iv_bytes(prot[mp4::kProtWords + mp4::kPrIvSize])};
  // the two track_IDs are all the walk needs of the track rows
  int64_t tracks[mp4::kTracks * mp4::kTrackWords] = {};
  tracks[mp4::kTkId] = a.info[static_cast<int64_t>(seg) * ts::kInfoWords + ts::kVideoPid];
  tracks[mp4::kTrackWords + mp4::kTkId] = a.info[static_cast<int64_t>(seg) * ts::kInfoWords + ts::kAudioPid];

  // ---- a. no sample has auxiliary data yet; lane 0 walks the top level
  for (int t = 0; t < mp4::kTracks; ++t) {
    v4i* aux = cbcs_aux(a, seg, t);
    for (int64_t k = tid; k < rec[t]; k += kCbThreads) aux[k] = v4i{-1, 0, -1, 0};
  }
  s_lo[tid] = 0x7fffffff;
  s_hi[tid] = -1;
  if (tid == 0) {
    s_status = 0;
    s_nsenc = 0;
    s_samples[0] = s_samples[1] = 0;
    s_blocks[0] = s_blocks[1] = 0;
    const mp4::TopOut top = mp4::top_walk(
        rd, n,
        [&](int64_t k, int64_t p, const mp4::Box& b) {
          if (k >= mp4::kMaxBoxRows) return;
          s_moof_p[k] = static_cast<int>(p);
          s_moof_hdr[k] = static_cast<int>(b.hdr);
          s_moof_size[k] = static_cast<int>(b.size);
        },
        [](int64_t, int64_t, const mp4::Box&) {});
    s_nm = static_cast<int>(top.n_moof < mp4::kMaxBoxRows ? top.n_moof : mp4::kMaxBoxRows);
  }
  __syncthreads();

  // ---- b. a lane per moof: the senc entries of its trafs' recorded samples
  if (tid < s_nm) {
    int lo = 0, hi = nr;  // the moof's first row of runs: rows ascend by moof
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (runs[mid * mp4::kRunWords + mp4::kRnMoof] < tid) lo = mid + 1;
      else hi = mid;
    }
    const int base = lo;
    int st = 0, n_senc = 0;
    const mp4::Box mb = {true, mp4::kMoof, s_moof_hdr[tid], s_moof_size[tid]};
    mp4::senc_walk(rd, s_moof_p[tid], mb, tracks, n,
                   [&](int slot, int64_t j0, int64_t cnt, int64_t sp, const mp4::Box& sb) {
      const int64_t g0 = base + j0;
      if (!prot_on[slot] || sp < 0 || g0 >= nr || runs[g0 * mp4::kRunWords + mp4::kRnMoof] != tid) return;
      ++n_senc;
      const mp4::SencHead h = mp4::senc_head(rd, sp, sb);
      if (!h.ok) {
        st |= static_cast<int>(mp4::kCbBadSenc);
        return;
      }
      v4i* aux = cbcs_aux(a, seg, slot);
      int64_t e = 0, q = h.at;
      bool more = true;
      for (int64_t g = g0; more && g < g0 + cnt && g < nr; ++g) {
        const int64_t first = runs[g * mp4::kRunWords + mp4::kRnFirst], count = runs[g * mp4::kRunWords + mp4::kRnCount];
        for (int64_t j = 0; j < count; ++j, ++e) {
          const int64_t k = first + j;
          if (e >= h.count || k >= rec[slot]) {  // samples ascend over the traf's runs
            more = false;
            break;
          }
          int64_t nsub;
          const int64_t next = mp4::senc_entry(rd, q, h.end, iv_size[slot], (h.flags & 2) != 0, nsub);
          if (next < 0) {
            st |= static_cast<int>(mp4::kCbBadSenc);
            more = false;
            break;
          }
          aux[k] = v4i{static_cast<int>(q), static_cast<int>(nsub), static_cast<int>(g), 0};
          q = next;
        }
      }
    });
    if (st) atomicOr(&s_status, st);
    if (n_senc) atomicAdd(&s_nsenc, n_senc);
  }
  __syncthreads();  // the aux rows are visible to the workgroup

  // ---- c. the byte span of each run over its samples that have an entry; a lane per run tests
  // its span against the runs in front of it
  const int64_t M = rec[0] + rec[1];
  for (int64_t i = tid; i < M; i += kCbThreads) {
    const int t = i >= rec[0] ? 1 : 0;
    const int64_t k = i - (t ? rec[0] : 0);
    const v4i ax = cbcs_aux(a, seg, t)[k];
    if (ax.x < 0 || ax.z < 0 || ax.z >= nr) continue;
    const int64_t o = clamp(cbcs_pes(a, seg, t)[ts::kPesWords * k + ts::kPesEsOffset], 0, n);
    const int64_t z = clamp(cbcs_msamples(a, seg, t)[k][mp4::kMsSize], 0, n - o);
    if (z > 0) {
      atomicMin(&s_lo[ax.z], static_cast<int>(o));
      atomicMax(&s_hi[ax.z], static_cast<int>(o + z));
    }
  }
  __syncthreads();
  {
    int shadow = 0;
    if (tid < nr)
      for (int r = 0; r < tid; ++r) shadow |= mp4::spans_meet(s_lo[r], s_hi[r], s_lo[tid], s_hi[tid]) ? 1 : 0;
    s_shadow[tid] = shadow;
  }
  __syncthreads();

  // ---- d. rounds of 256 samples with a carry, the video track first
  long long carry_r = 0, carry_b = 0;
  int st = 0;
  for (int64_t base = 0; base < M; base += kCbThreads) {
    const int64_t i = base + tid;
    const bool valid = i < M;
    const int t = valid && i >= rec[0] ? 1 : 0;
    const int64_t k = i - (t ? rec[0] : 0);
    const int64_t c = prot[t * mp4::kProtWords + mp4::kPrCrypt], s = prot[t * mp4::kProtWords + mp4::kPrSkip];
    long long n_rng = 0, n_blk = 0;
    int64_t o = 0, z = 0, sub = 0, nsub = -1;
    bool live = false;
    if (valid) {
      const v4i ax = cbcs_aux(a, seg, t)[k];
      o = clamp(cbcs_pes(a, seg, t)[ts::kPesWords * k + ts::kPesEsOffset], 0, n);
      z = clamp(cbcs_msamples(a, seg, t)[k][mp4::kMsSize], 0, n - o);
      if (ax.x < 0 || ax.z < 0 || ax.z >= nr) {
        st |= static_cast<int>(mp4::kCbNoSenc);
      } else if (s_shadow[ax.z]) {
        st |= static_cast<int>(mp4::kCbOverlap);
      } else {
        live = true;
        sub = ax.x + iv_size[t] + 2;
        nsub = ax.y;
        const bool ok = mp4::sample_ranges(rd, o, z, sub, nsub, [&](int64_t, int64_t len) {
          const int64_t b = mp4::cipher_blocks(len, c, s);
          if (b > 0) {
            ++n_rng;
            n_blk += b;
          }
        });
        if (!ok) st |= static_cast<int>(mp4::kCbBadSenc);
      }
    }
    const WgPrefix<long long> pr = wg_exclusive_prefix<kCbWaves>(wave_scan64(n_rng), n_rng, s_wave0);
    const WgPrefix<long long> pb = wg_exclusive_prefix<kCbWaves>(wave_scan64(n_blk), n_blk, s_wave1);
    if (live && n_rng > 0) {
      long long rank_r = carry_r + pr.before, rank_b = carry_b + pb.before;
      mp4::sample_ranges(rd, o, z, sub, nsub, [&](int64_t off, int64_t len) {
        const int64_t b = mp4::cipher_blocks(len, c, s);
        if (b <= 0) return;
        if (rank_r < max_range)
          rows[rank_r] = v4i{static_cast<int>(off), static_cast<int>(len),
                             static_cast<int>((t << mp4::kRgTrackShift) | k), static_cast<int>(rank_b)};
        ++rank_r;
        rank_b += b;
      });
      atomicAdd(&s_samples[t], 1);
      atomicAdd(&s_blocks[t], static_cast<unsigned long long>(n_blk));
    }
    carry_r += pr.total;
    carry_b += pb.total;
    __syncthreads();  // s_wave0, s_wave1 are free again
  }
  if (st) atomicOr(&s_status, st);
  __syncthreads();

  // ---- e. the rows beyond, cinfo
  const int64_t n_rec = carry_r < max_range ? carry_r : max_range;
  for (int64_t i = n_rec + tid; i < max_range; i += kCbThreads) rows[i] = v4i{-1, -1, -1, -1};
  if (tid == 0) {
    const int64_t status = s_status | damaged | (carry_r > max_range ? mp4::kCbRangeOverflow : 0);
    ci[0] = v2l{status, carry_r};
    ci[1] = v2l{s_samples[0], s_samples[1]};
    ci[2] = v2l{static_cast<long long>(s_blocks[0]), static_cast<long long>(s_blocks[1])};
    ci[3] = v2l{s_nsenc, 0};
  }
}
static_assert(mp4::kCbStatus == 0 && mp4::kCbNumRanges == 1 && mp4::kCbVideoSamples == 2 && mp4::kCbAudioSamples == 3 &&
                  mp4::kCbVideoBlocks == 4 && mp4::kCbAudioBlocks == 5 && mp4::kCbNumSenc == 6,
              "cbcs_plan_kernel writes cinfo two words per store");

// ---------------------------------------------------------------- 2. decrypt
// 16 bytes with the widest stores the address allows
__device__ __forceinline__ void cbcs_store16(uint8_t* p, const uint4& v) {
  const uint32_t w[4] = {v.x, v.y, v.z, v.w};
  const uintptr_t al = reinterpret_cast<uintptr_t>(p);
  if (!(al & 15)) {
    *reinterpret_cast<uint4*>(p) = v;
  } else if (!(al & 7)) {
    reinterpret_cast<uint2*>(p)[0] = uint2{v.x, v.y};
    reinterpret_cast<uint2*>(p)[1] = uint2{v.z, v.w};
  } else if (!(al & 3)) {
#pragma unroll
    for (int d = 0; d < 4; ++d) reinterpret_cast<uint32_t*>(p)[d] = w[d];
  } else if (!(al & 1)) {
#pragma unroll
    for (int d = 0; d < 8; ++d) reinterpret_cast<uint16_t*>(p)[d] = static_cast<uint16_t>(w[d >> 1] >> (16 * (d & 1)));
  } else {
#pragma unroll
    for (int d = 0; d < 16; ++d) p[d] = static_cast<uint8_t>(w[d >> 2] >> (8 * (d & 3)));
  }
}

// largest row in [0, K) whose rank is <= j; ranks ascend and the first is 0
__device__ __forceinline__ int cbcs_last_le(const v4i* rows, int K, int j) {
  int lo = 0, hi = K;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (rows[mid].w <= j) lo = mid;
    else hi = mid;
  }
  return lo;
}

__global__ __launch_bounds__(kCbThreads) void cbcs_blocks_kernel(CbcsArgs a) {
  __shared__ AesSmallLds s_aes;
  __shared__ v4i s_rows[kCbThreads];
  const int seg = blockIdx.y, tid = threadIdx.x;
  if (!a.enable[seg]) return;
  const int64_t* ci = a.cinfo + static_cast<int64_t>(seg) * mp4::kCbInfoWords;
  const int n_rec = static_cast<int>(clamp(ci[mp4::kCbNumRanges], 0, a.max_range));
  if (n_rec == 0) return;
  const v4i* rows = reinterpret_cast<const v4i*>(a.ranges + table_words(seg, a.max_range, mp4::kRangeWords));
  const int64_t* prot = a.prot + static_cast<int64_t>(seg) * mp4::kTracks * mp4::kProtWords;
  const v4i last = rows[n_rec - 1];
  const int64_t* lp = prot + ((last.z >> mp4::kRgTrackShift) & 1) * mp4::kProtWords;
  const int total = static_cast<int>(last.w + mp4::cipher_blocks(last.y, lp[mp4::kPrCrypt], lp[mp4::kPrSkip]));
  if (static_cast<int64_t>(blockIdx.x) * kCbThreads >= total) return;  // before the first barrier

  aes_small_fill(s_aes, a.td, a.isb, a.round_keys + static_cast<int64_t>(seg) * es::kAesRoundKeyWords, tid);
  const int n = cbcs_segment_bytes(a, seg);
  const __amdgpu_buffer_rsrc_t rsrc = mp4_reader(a.src, a.src_numel, a.src_off[seg], n).rsrc;
  uint8_t* out = a.dst + a.dst_off[seg];
  for (int64_t t0 = static_cast<int64_t>(blockIdx.x) * kCbThreads; t0 < total;
       t0 += static_cast<int64_t>(gridDim.x) * kCbThreads) {
    const int j0 = static_cast<int>(t0), j1 = j0 + kCbThreads - 1 < total - 1 ? j0 + kCbThreads - 1 : total - 1;
    const int lo = cbcs_last_le(rows, n_rec, j0), hi = cbcs_last_le(rows, n_rec, j1);
    if (tid <= hi - lo) s_rows[tid] = rows[lo + tid];  // every row but the first starts inside the tile: at most 256
    __syncthreads();  // also: s_aes is filled
    const int j = j0 + tid;
    if (j < total) {
      const v4i r = s_rows[cbcs_last_le(s_rows, hi - lo + 1, j)];
      const int t = (r.z >> mp4::kRgTrackShift) & 1, sample = r.z & ((1 << mp4::kRgTrackShift) - 1);
      const int64_t* p = prot + t * mp4::kProtWords;
      const int64_t c = p[mp4::kPrCrypt], s = p[mp4::kPrSkip];
      const int jj = j - r.w;
      const int64_t at = r.x + mp4::cipher_block_at(jj, c, s);
      if (at >= 0 && at + 16 <= n && at + 16 <= static_cast<int64_t>(r.x) + r.y) {  // what the plan guarantees
        const v4u cj = load16_unaligned(rsrc, static_cast<int>(at));
        v4u prev;
        if (jj > 0) {
          prev = load16_unaligned(rsrc, static_cast<int>(r.x + mp4::cipher_block_at(jj - 1, c, s)));
        } else {
          const int ivs = mp4::iv_bytes(p[mp4::kPrIvSize]);
          if (ivs > 0) {
            prev = load16_unaligned(rsrc, cbcs_aux(a, seg, t)[sample].x);
            if (ivs == 8) prev.z = prev.w = 0;
          } else {
            const uint8_t* iv = mp4::iv_bytes(p[mp4::kPrConstIvSize]) > 0
                                    ? a.const_iv + (static_cast<int64_t>(seg) * mp4::kTracks + t) * es::kAesBlock
                                    : a.iv + static_cast<int64_t>(seg) * es::kAesBlock;
            prev = *reinterpret_cast<const v4u*>(iv);
          }
        }
        const uint4 d = aes_small_decrypt(s_aes, uint4{cj.x, cj.y, cj.z, cj.w});
        cbcs_store16(out + at, uint4{d.x ^ prev.x, d.y ^ prev.y, d.z ^ prev.z, d.w ^ prev.w});
      }
    }
    __syncthreads();  // s_rows is free again
  }
}

hipError_t launch_cbcs(const CbcsArgs& a) {
  if (a.nseg <= 0) return hipSuccess;
  if (a.nseg > 65535 || !mp4::max_range_ok(a.max_range) || a.max_pes <= 0 || a.max_pes >= (int64_t(1) << mp4::kRgTrackShift) ||
      !mp4::max_rows_ok(a.max_run) || a.max_blocks < 0 || a.max_blocks > 0x7fffffff / 16)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(cbcs_plan_kernel, dim3(a.nseg), dim3(kCbThreads), 0, a.stream, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess || a.max_blocks == 0) return e;
  const int64_t tiles = (a.max_blocks + kCbThreads - 1) / kCbThreads;
  hipLaunchKernelGGL(cbcs_blocks_kernel, dim3(static_cast<unsigned>(tiles < kCbGridTiles ? tiles : kCbGridTiles), a.nseg),
                     dim3(kCbThreads), 0, a.stream, a);
  return hipGetLastError();
}

}  // namespace dev
}  // namespace hlsp2p
