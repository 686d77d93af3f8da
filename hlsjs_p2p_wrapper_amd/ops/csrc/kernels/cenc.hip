// cenc (ISO/IEC 23001-7 AES-128-CTR, HLS SAMPLE-AES-CTR on fragmented MP4) decryption of a demuxed
// batch into a copy (docs/CENC.md) — CDNA4 / gfx950.
//
// Input: as cbcs.hip, with the forward round keys, TeL and the S-box in place of the inverse ones.
// Output, identical to the host implementation runtime/cenc.cpp cenc_segment:
//   dst:    every byte of every recorded range XORed with its keystream byte, nothing else touched
//   ranges: int32[seg][max_range][kCnRangeWords]    cinfo: int64[seg][kCnInfoWords]
//
// Two launches on the caller's stream, ordered by the stream alone; no workgroup waits for another:
//   1. cenc_plan_kernel — protected_plan_dev.h with the cenc range and unit rules: a range is
//      recorded from one byte on, its units are the keystream blocks it touches, and its row also
//      carries its position in the sample's keystream and where the sample's IV stands.
//   2. cenc_units_kernel — 1024-thread workgroups, one per CU, each with the bulk decrypt's 160 KiB
//      conflict-free image (aes_dev.h) filled with the forward tables (aes_enc_dev.h).  The grid is
//      persistent over pairs (segment, tile of kCnTileUnits consecutive unit ranks): workgroup g
//      takes pairs g, g + gridDim.x, ...; a pair beyond its segment's units is skipped.  A lane
//      takes kCnLaneUnits units of the tile, 1024 apart, so the round pipeline has independent
//      blocks and a wave's loads and stores are contiguous.  The image leaves no LDS for the rows:
//      the tile's rows are narrowed by two workgroup-uniform searches at the tile's ends, a lane
//      finds the rows of its units among them in global memory (L1 / L2 hits), the searches of a
//      group step by step together.  Per unit: the counter block from
//      the IV (a 16-byte unaligned load through the segment's buffer range, or the descriptor's),
//      ten rounds, the ciphertext from the SOURCE, the XOR, and a store of the bytes inside the
//      range into the copy.  The segment's round keys sit in SGPRs and are reloaded when the
//      pair's segment changes.
// Segments that did not ask and segments without a protected track cost a pair's test.  The source
// is never written.  All stores are vector stores from plain C++.
#include "aes_enc_dev.h"
#include "protected_plan_dev.h"

namespace hlsp2p {
namespace dev {

static_assert(mp4::kCnRangeWords == 8, "a ranges row is two 16-byte vectors");
static_assert(mp4::kCnTileUnits == kAesImageThreads * mp4::kCnLaneUnits, "a tile is kCnLaneUnits units per lane");
static_assert(mp4::kCnOffset == 0 && mp4::kCnLength == 1 && mp4::kCnSample == 2 && mp4::kCnRank == 3 &&
                  mp4::kCnStreamPos == 4 && mp4::kCnIvOffset == 5,
              "CencPlan::write and cenc_units_kernel take a row as two vectors");

// ---------------------------------------------------------------- 1. plan (protected_plan_dev.h)
struct CencPlan {
  static constexpr int kRowVecs = 2;
  static constexpr bool kUnitsInInfo = true, kSumIsUnits = false;
  static __device__ __forceinline__ int64_t units(int64_t len, int64_t p0, int64_t, int64_t) {
    return mp4::ctr_units(p0, len);
  }
  static __device__ __forceinline__ void write(v4i* row, int off, int len, int sample, int rank, int p0, int iv_off) {
    row[0] = v4i{off, len, sample, rank};
    row[1] = v4i{p0, iv_off, 0, 0};
  }
};
__global__ __launch_bounds__(kCbThreads) void cenc_plan_kernel(CbcsArgs a) { protected_plan<CencPlan>(a); }

// ---------------------------------------------------------------- 2. units
// at[i] = the largest row in [0, K) whose rank is <= u[i]; ranks ascend and the first is 0.  The N
// searches go step by step together, so a step's N loads are in flight at once: the latency of
// dependent loads, not their number, is what a search costs here
template <int N>
__device__ __forceinline__ void cenc_last_le(const v4i* rows, int K, const int (&u)[N], int (&at)[N]) {
#pragma unroll
  for (int i = 0; i < N; ++i) at[i] = 0;
  for (int len = K; len > 1;) {  // the answer of search i lies in [at[i], at[i] + len)
    const int half = len >> 1;
    int r[N];
#pragma unroll
    for (int i = 0; i < N; ++i) r[i] = rows[2 * (at[i] + half)].w;
#pragma unroll
    for (int i = 0; i < N; ++i) at[i] += r[i] <= u[i] ? half : 0;
    len -= half;
  }
}

__global__ __launch_bounds__(kAesImageThreads, 1) void cenc_units_kernel(CbcsArgs a, int tiles_per_seg, int64_t pairs) {
  __shared__ uint32_t s_tab[kTdDwords + kIsDwords];  // 160 KiB (aes_cbc.hip's layout)
  constexpr int kN = mp4::kCnLaneUnits, kT = mp4::kCnTileUnits;
  const int tid = threadIdx.x;
  aes_image_fill(s_tab, a.td, a.isb, tid);
  __syncthreads();
  const uint8_t* s_bytes = reinterpret_cast<const uint8_t*>(s_tab);
  uint32_t td_base[4], is_base;
  aes_image_bases(tid, td_base, is_base);

  int cur = -1;
  uint32_t rk[44];
  for (int64_t x = blockIdx.x; x < pairs; x += gridDim.x) {
    const int seg = static_cast<int>(x / tiles_per_seg), tile = static_cast<int>(x % tiles_per_seg);
    if (!a.enable[seg]) continue;
    const int64_t* ci = a.cinfo + static_cast<int64_t>(seg) * mp4::kCnInfoWords;
    const int n_rec = static_cast<int>(clamp(ci[mp4::kCnNumRanges], 0, a.max_range));
    if (n_rec == 0) continue;
    const v4i* rows = reinterpret_cast<const v4i*>(a.ranges + table_words(seg, a.max_range, mp4::kCnRangeWords));
    // the units of the recorded ranges: cinfo's total also counts the unrecorded ones
    const int total = static_cast<int>(rows[2 * (n_rec - 1)].w +
                                       mp4::ctr_units(rows[2 * (n_rec - 1) + 1].x, rows[2 * (n_rec - 1)].y));
    const int t0 = tile * kT;
    if (t0 >= total) continue;
    const int t1 = t0 + kT - 1 < total - 1 ? t0 + kT - 1 : total - 1;
    // no unit for this wave (no barrier follows); wave-uniform by construction, and said so, or the
    // round keys below would be carried in VGPRs
    if (__builtin_amdgcn_readfirstlane(t0 + (tid & ~63) > t1 ? 1 : 0)) continue;
    if (seg != cur) {
      cur = seg;
#pragma unroll
      for (int k = 0; k < 44; ++k)
        rk[k] = __builtin_amdgcn_readfirstlane(a.round_keys[static_cast<int64_t>(seg) * es::kAesRoundKeyWords + k]);
    }
    const int n = cbcs_segment_bytes(a, seg);
    SegReader rd = mp4_reader(a.src, a.src_numel, a.src_off[seg], n);
    uint8_t* out = a.dst + a.dst_off[seg];
    const int64_t* prot = a.prot + static_cast<int64_t>(seg) * mp4::kTracks * mp4::kProtWords;
    const int ends[2] = {t0, t1};
    int span[2];  // the tile's first and last row
    cenc_last_le(rows, n_rec, ends, span);
    int unit[kN], idx[kN];  // a lane's units (one beyond the tile looks for the tile's last) and their rows
#pragma unroll
    for (int i = 0; i < kN; ++i) unit[i] = t0 + i * kAesImageThreads + tid < t1 ? t0 + i * kAesImageThreads + tid : t1;
    cenc_last_le(rows + 2 * span[0], span[1] - span[0] + 1, unit, idx);

    uint32_t st[kN][4];
    int at[kN], cut[kN];  // the unit's keystream block lies at at; cut = first | behind-last << 8 of its bytes inside the range
#pragma unroll
    for (int i = 0; i < kN; ++i) {
      const int u = t0 + i * kAesImageThreads + tid;
      st[i][0] = st[i][1] = st[i][2] = st[i][3] = 0;
      at[i] = cut[i] = 0;
      if (u <= t1) {
        const v4i r0 = rows[2 * (span[0] + idx[i])], r1 = rows[2 * (span[0] + idx[i]) + 1];
        const int t = (r0.z >> mp4::kRgTrackShift) & 1;
        const int64_t j = mp4::ctr_unit_block(r1.x, u - r0.w);
        const int64_t f = mp4::ctr_block_at(r0.x, r1.x, j);
        const int64_t fl = f > r0.x ? f : r0.x, fh = f + 16 < static_cast<int64_t>(r0.x) + r0.y ? f + 16 : static_cast<int64_t>(r0.x) + r0.y;
        if (fl >= 0 && fh <= n && fl < fh && f > -16) {  // what the plan guarantees
          at[i] = static_cast<int>(f);
          cut[i] = static_cast<int>(fl - f) | (static_cast<int>(fh - f) << 8);
          const int64_t* p = prot + t * mp4::kProtWords;
          v4u iv;
          if (r1.y >= 0) {
            iv = load16_unaligned(rd.rsrc, r1.y);
            if (mp4::iv_bytes(p[mp4::kPrIvSize]) == 8) iv.z = iv.w = 0;
          } else {
            const uint8_t* q = mp4::iv_bytes(p[mp4::kPrConstIvSize]) > 0
                                   ? a.const_iv + (static_cast<int64_t>(seg) * mp4::kTracks + t) * es::kAesBlock
                                   : a.iv + static_cast<int64_t>(seg) * es::kAesBlock;
            iv = *reinterpret_cast<const v4u*>(q);
          }
          const uint32_t ivw[4] = {iv.x, iv.y, iv.z, iv.w};
          uint32_t cw[4];
          mp4::ctr_block(ivw, j, cw);
#pragma unroll
          for (int w = 0; w < 4; ++w) st[i][w] = cw[w] ^ rk[w];
        }
      }
    }
    AES_ENC_ROUNDS_PIPELINED(kN, st, rk)
    // the ciphertext of the whole units: in flight during the last round (loading it ahead of the
    // rounds, as the bulk decrypt does, costs 16 registers that the kernel does not have)
    v4u c[kN];
#pragma unroll
    for (int i = 0; i < kN; ++i) c[i] = cut[i] == 16 << 8 ? load16_unaligned(rd.rsrc, at[i]) : v4u{0, 0, 0, 0};
#pragma unroll
    for (int i = 0; i < kN; ++i) {
      uint32_t ks[4];
      AES_ENC_FINAL(st[i][0], st[i][1], st[i][2], st[i][3], ks[0], ks[1], ks[2], ks[3], rk + 40)
      if (cut[i] == 16 << 8) {
        cbcs_store16(out + at[i], uint4{c[i].x ^ ks[0], c[i].y ^ ks[1], c[i].z ^ ks[2], c[i].w ^ ks[3]});
      } else if (cut[i] != 0) {  // a unit cut by its range's ends: byte by byte
        SegReader bytes = rd;
#pragma unroll
        for (int d = 0; d < 16; ++d)
          if (d >= (cut[i] & 0xff) && d < (cut[i] >> 8))
            out[at[i] + d] = static_cast<uint8_t>(bytes.u8(at[i] + d) ^ ((ks[d >> 2] >> (8 * (d & 3))) & 0xffu));
      }
    }
  }
}

hipError_t launch_cenc(const CencArgs& c) {
  const CbcsArgs& a = c.t;
  if (a.nseg <= 0) return hipSuccess;
  if (a.nseg > 65535 || !mp4::max_range_ok(a.max_range) || a.max_pes <= 0 || a.max_pes >= (int64_t(1) << mp4::kRgTrackShift) ||
      !mp4::max_rows_ok(a.max_run) || c.max_cap < 0 || c.max_cap >= 0x7fffffff - 64 || c.num_cu <= 0)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(cenc_plan_kernel, dim3(a.nseg), dim3(kCbThreads), 0, a.stream, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess || c.max_cap == 0) return e;
  const int64_t tiles = (mp4::cenc_unit_bound(c.max_cap, a.max_range) + mp4::kCnTileUnits - 1) / mp4::kCnTileUnits;
  const int64_t pairs = tiles * a.nseg;
  hipLaunchKernelGGL(cenc_units_kernel, dim3(static_cast<unsigned>(pairs < c.num_cu ? pairs : c.num_cu)),
                     dim3(kAesImageThreads), 0, a.stream, a, static_cast<int>(tiles), pairs);
  return hipGetLastError();
}

}  // namespace dev
}  // namespace hlsp2p
