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
#include "protected_plan_dev.h"

namespace hlsp2p {
namespace dev {

// grid.x of the decrypt: the host knows only cap / 16, an upper bound of a segment's cipher blocks;
// beyond this many tiles a workgroup takes several
constexpr int kCbGridTiles = 64;
static_assert(mp4::kCbTileBlocks == kCbThreads, "a lane per cipher block of a tile");
static_assert(mp4::kRangeWords == 4, "16-byte rows");

// ---------------------------------------------------------------- 1. plan (protected_plan_dev.h)
struct CbcsPlan {
  static constexpr int kRowVecs = 1;
  static constexpr bool kUnitsInInfo = false, kSumIsUnits = true;
  static __device__ __forceinline__ int64_t units(int64_t len, int64_t, int64_t c, int64_t s) {
    return mp4::cipher_blocks(len, c, s);
  }
  static __device__ __forceinline__ void write(v4i* row, int off, int len, int sample, int rank, int, int) {
    row[0] = v4i{off, len, sample, rank};
  }
};
__global__ __launch_bounds__(kCbThreads) void cbcs_plan_kernel(CbcsArgs a) { protected_plan<CbcsPlan>(a); }

// ---------------------------------------------------------------- 2. decrypt
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
