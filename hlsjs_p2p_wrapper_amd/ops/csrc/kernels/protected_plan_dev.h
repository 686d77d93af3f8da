// The plan kernel that cbcs.hip and cenc.hip share, as a template over the scheme: one 256-thread
// workgroup per segment walks the senc boxes of a demuxed fragmented-MP4 segment, applies the
// overlap rule and ranks every protected range and every unit of cipher work (docs/CBCS.md,
// docs/CENC.md).  The scheme says what a range's units are and what its row looks like:
//   kRowVecs                 16-byte vectors per ranges row
//   kUnitsInInfo             the total of the units goes into the last cinfo word
//   kSumIsUnits              the per-track sum is the sum of the units (else of the range lengths)
//   units(len, p0, c, s)     units of a range of len bytes at byte p0 of the sample's protected bytes
//   write(row, off, len, sample, rank, p0, iv_off)
// The senc, subsample and overlap rules are shared/grammar.hpp (namespace mp4).
#pragma once
#include "launch.h"
#include "mp4_dev.h"

namespace hlsp2p {
namespace dev {

constexpr int kCbThreads = 256;
constexpr int kCbWaves = kCbThreads / 64;
static_assert(mp4::kMaxBoxRows == kCbThreads, "a lane per moof or run row in one round");
static_assert(mp4::kAuxWords == 4 && mp4::kCbInfoWords == 8 && mp4::kCnInfoWords == 8, "16-byte rows");

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

template <class Scheme>
__device__ __forceinline__ void protected_plan(const CbcsArgs& a) {
  __shared__ long long s_wave0[kCbWaves], s_wave1[kCbWaves];
  __shared__ unsigned long long s_blocks[mp4::kTracks];
  __shared__ int s_moof_p[mp4::kMaxBoxRows], s_moof_hdr[mp4::kMaxBoxRows], s_moof_size[mp4::kMaxBoxRows];
  __shared__ int s_lo[mp4::kMaxBoxRows], s_hi[mp4::kMaxBoxRows], s_shadow[mp4::kMaxBoxRows];
  __shared__ int s_nm, s_status, s_nsenc, s_samples[mp4::kTracks];
  constexpr int kRow = Scheme::kRowVecs;
  const int seg = blockIdx.x, tid = threadIdx.x;
  const int64_t max_range = a.max_range, max_pes = a.max_pes;
  v4i* rows = reinterpret_cast<v4i*>(a.ranges + table_words(seg, max_range, 4 * kRow));
  v2l* ci = reinterpret_cast<v2l*>(a.cinfo + static_cast<int64_t>(seg) * mp4::kCbInfoWords);
  const int64_t* prot = a.prot + static_cast<int64_t>(seg) * mp4::kTracks * mp4::kProtWords;
  const int64_t* mi = a.minfo + static_cast<int64_t>(seg) * mp4::kMinfoWords;
  const bool on = a.enable[seg] != 0;
  const bool prot_on[mp4::kTracks] = {on && prot[mp4::kPrProtected] == 1,
                                      on && prot[mp4::kProtWords + mp4::kPrProtected] == 1};
  const int64_t damaged = on && (mi[mp4::kMStatus] & mp4::kCbDamagedMask) ? mp4::kCbDemuxDamaged : 0;
  if (!prot_on[0] && !prot_on[1]) {  // before the first barrier
    for (int64_t i = tid; i < max_range * kRow; i += kCbThreads) rows[i] = v4i{-1, -1, -1, -1};
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
    long long n_rng = 0, n_blk = 0, n_sum = 0;
    int64_t o = 0, z = 0, sub = 0, nsub = -1;
    int iv_off = -1;
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
        iv_off = iv_size[t] > 0 ? ax.x : -1;
        int64_t p0 = 0;
        const bool ok = mp4::sample_ranges(rd, o, z, sub, nsub, [&](int64_t, int64_t len) {
          const int64_t b = Scheme::units(len, p0, c, s);
          if (b > 0) {
            ++n_rng;
            n_blk += b;
          }
          p0 += len;
        });
        n_sum = Scheme::kSumIsUnits ? n_blk : p0;
        if (!ok) st |= static_cast<int>(mp4::kCbBadSenc);
      }
    }
    const WgPrefix<long long> pr = wg_exclusive_prefix<kCbWaves>(wave_scan64(n_rng), n_rng, s_wave0);
    const WgPrefix<long long> pb = wg_exclusive_prefix<kCbWaves>(wave_scan64(n_blk), n_blk, s_wave1);
    if (live && n_rng > 0) {
      long long rank_r = carry_r + pr.before, rank_b = carry_b + pb.before;
      int64_t p0 = 0;
      mp4::sample_ranges(rd, o, z, sub, nsub, [&](int64_t off, int64_t len) {
        const int64_t b = Scheme::units(len, p0, c, s);
        if (b > 0) {
          if (rank_r < max_range)
            Scheme::write(rows + rank_r * kRow, static_cast<int>(off), static_cast<int>(len),
                          static_cast<int>((t << mp4::kRgTrackShift) | k), static_cast<int>(rank_b),
                          static_cast<int>(p0), iv_off);
          ++rank_r;
          rank_b += b;
        }
        p0 += len;
      });
      atomicAdd(&s_samples[t], 1);
      atomicAdd(&s_blocks[t], static_cast<unsigned long long>(n_sum));
    }
    carry_r += pr.total;
    carry_b += pb.total;
    __syncthreads();  // s_wave0, s_wave1 are free again
  }
  if (st) atomicOr(&s_status, st);
  __syncthreads();

  // ---- e. the rows beyond, cinfo
  const int64_t n_rec = carry_r < max_range ? carry_r : max_range;
  for (int64_t i = n_rec * kRow + tid; i < max_range * kRow; i += kCbThreads) rows[i] = v4i{-1, -1, -1, -1};
  if (tid == 0) {
    const int64_t status = s_status | damaged | (carry_r > max_range ? mp4::kCbRangeOverflow : 0);
    ci[0] = v2l{status, carry_r};
    ci[1] = v2l{s_samples[0], s_samples[1]};
    ci[2] = v2l{static_cast<long long>(s_blocks[0]), static_cast<long long>(s_blocks[1])};
    ci[3] = v2l{s_nsenc, Scheme::kUnitsInInfo ? carry_b : 0};
  }
}
static_assert(mp4::kCbStatus == 0 && mp4::kCbNumRanges == 1 && mp4::kCbVideoSamples == 2 && mp4::kCbAudioSamples == 3 &&
                  mp4::kCbVideoBlocks == 4 && mp4::kCbAudioBlocks == 5 && mp4::kCbNumSenc == 6,
              "protected_plan writes cinfo two words per store");
static_assert(mp4::kCnStatus == 0 && mp4::kCnNumRanges == 1 && mp4::kCnVideoSamples == 2 && mp4::kCnAudioSamples == 3 &&
                  mp4::kCnVideoBytes == 4 && mp4::kCnAudioBytes == 5 && mp4::kCnNumSenc == 6 && mp4::kCnNumUnits == 7,
              "protected_plan writes cinfo two words per store");

}  // namespace dev
}  // namespace hlsp2p
