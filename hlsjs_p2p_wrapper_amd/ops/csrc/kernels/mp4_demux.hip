// Demux of fragmented-MP4 (CMAF) media segments (docs/FMP4DEMUX.md) — CDNA4 / gfx950.
//
// Input: the segments where the decrypt left them, only read, and per segment two track rows.
// Output per segment, identical to the host implementation runtime/mp4.cpp demux_segment:
//   minfo: int64[seg][kMinfoWords]            msamples: int32[seg][2][max_pes][kMsampleWords]
//   runs:  int64[seg][max_run][kRunWords]     emsg:     int64[seg][max_emsg][kEmsgWords]
//   info / pes in the layout of ts_demux.hip, nal / au / aframes / sinfo in that of es_index.hip
//
// These are latency chains over a few KB of boxes.  Three launches on the caller's stream, ordered
// by the stream alone, one 256-thread workgroup per segment each; no workgroup waits for another:
//   1. mp4_boxes_kernel — lane 0 walks the top level (the one serial chain: a 16-byte load per
//      box); a lane per recorded moof walks its children twice, to count its runs and, behind a
//      workgroup scan of the counts, to record them in order into LDS; the top lanes parse an emsg
//      each meanwhile.  A lane per run then gets its first sample from two 64-bit scans of the
//      counts and finds its two anchor runs by walking back over LDS; the rows leave LDS 16 bytes
//      per store.
//   2. mp4_samples_kernel — per track, rounds of 256 samples with a carry: a lane finds its run by
//      binary search over the LDS copy of the track's first-sample column, reads its entry with one
//      16-byte load, and two 64-bit workgroup scans (sizes, durations) give offset and decode time
//      as "scan value minus the scan value at the anchor run's first sample", which the lanes of
//      the runs that start in the round leave in LDS.  Writes pes, msamples, minfo's track words
//      and info.
//   3. mp4_nal_kernel — a lane per recorded video sample walks its length-prefixed NAL units twice:
//      to count them and, behind a workgroup scan, to write the nal rows; then au, sinfo, the fills.
// Every byte of a segment is read through a buffer resource that ends with the segment (rounded up
// to a dword, never beyond the tensor): a box header at any alignment or ending at the segment's
// last byte is safe, and a read the rules do not allow would return 0, not fault.
// All byte rules are shared/grammar.hpp (namespace mp4), the same functions runtime/mp4.cpp calls.
#include "launch.h"
#include "mp4_dev.h"

namespace hlsp2p {
namespace dev {

constexpr int kMp4Threads = 256;
constexpr int kMp4Waves = kMp4Threads / 64;
static_assert(mp4::kMaxBoxRows == kMp4Threads, "a lane per moof, run or emsg row in one round");
static_assert(mp4::kRunWords % 2 == 0 && mp4::kEmsgWords % 2 == 0, "run and emsg rows are 16-byte vectors");
static_assert(mp4::kMsampleWords == 4 && es::kNalWords == 4 && es::kAuWords == 4, "16-byte rows");

// Passed by value as the first kernel parameter.
struct Mp4View {
  const uint8_t* buf;
  int64_t buf_numel;
  const int64_t *off, *len, *cap, *tracks;
  mp4::Limits lim;
  mp4::Tables t;
};

// n = clamp(len, 0, cap), below 2^31
__device__ __forceinline__ int mp4_segment_bytes(const Mp4View& v, int seg) {
  return static_cast<int>(clamp(v.len[seg], 0, clamp(v.cap[seg], 0, 0x7fffffff)));
}

// the reader (mp4_dev.h) of segment seg of n bytes
__device__ __forceinline__ SegReader mp4_reader(const Mp4View& v, int seg, int n) {
  return mp4_reader(v.buf, v.buf_numel, v.off[seg], n);
}

__global__ __launch_bounds__(kMp4Threads) void mp4_boxes_kernel(Mp4View v) {
  __shared__ __attribute__((aligned(16))) long long s_run[mp4::kMaxBoxRows][mp4::kRunWords];
  __shared__ long long s_tracks[mp4::kTracks * mp4::kTrackWords];
  __shared__ long long s_first[mp4::kMaxBoxRows];
  __shared__ long long s_wave0[kMp4Waves], s_wave1[kMp4Waves];
  __shared__ long long s_seq;
  __shared__ int s_box_p[2][mp4::kMaxBoxRows], s_box_hdr[2][mp4::kMaxBoxRows], s_box_size[2][mp4::kMaxBoxRows];
  __shared__ int s_top[3];  // top-level status, moof and emsg boxes
  __shared__ int s_wave[kMp4Waves];
  __shared__ int s_status, s_other;
  const int seg = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
  const int n = mp4_segment_bytes(v, seg);
  const int max_moof = static_cast<int>(v.lim.max_moof), max_run = static_cast<int>(v.lim.max_run),
            max_emsg = static_cast<int>(v.lim.max_emsg);
  SegReader rd = mp4_reader(v, seg, n);
  if (tid < mp4::kTracks * mp4::kTrackWords) s_tracks[tid] = v.tracks[seg * mp4::kTracks * mp4::kTrackWords + tid];
  if (tid == 0) {
    s_status = 0;
    s_other = 0;
    s_seq = -1;
  }
  const int64_t* tracks = reinterpret_cast<const int64_t*>(s_tracks);

  // ---- a. the top level, one lane
  if (tid == 0) {
    auto keep = [&](int which, int limit) {
      return [=](int64_t k, int64_t p, const mp4::Box& b) {
        if (k >= limit) return;
        s_box_p[which][k] = static_cast<int>(p);
        s_box_hdr[which][k] = static_cast<int>(b.hdr);
        s_box_size[which][k] = static_cast<int>(b.size);
      };
    };
    const mp4::TopOut top = mp4::top_walk(rd, n, keep(0, max_moof), keep(1, max_emsg));
    s_top[0] = static_cast<int>(top.status);
    s_top[1] = static_cast<int>(top.n_moof);
    s_top[2] = static_cast<int>(top.n_emsg);
  }
  __syncthreads();
  const int n_moof = s_top[1], n_emsg = s_top[2];
  const int nm = n_moof < max_moof ? n_moof : max_moof, ne = n_emsg < max_emsg ? n_emsg : max_emsg;
  const bool moof_lane = tid < nm;
  const mp4::Box mb = {true, mp4::kMoof, moof_lane ? s_box_hdr[0][tid] : 8, moof_lane ? s_box_size[0][tid] : 8};
  const int64_t mp = moof_lane ? s_box_p[0][tid] : 0;

  // ---- b. a lane per moof counts its runs; the top lanes take an emsg each
  int my_runs = 0;
  if (moof_lane) {
    const mp4::MoofOut o = mp4::moof_walk(rd, mp, mb, tracks, n, [](int64_t, const mp4::Run&) {});
    my_runs = static_cast<int>(o.n_run);
    if (o.status) atomicOr(&s_status, static_cast<int>(o.status));
    if (o.n_other) atomicAdd(&s_other, static_cast<int>(o.n_other));
    if (tid == 0) s_seq = o.seq;
  }
  {
    const int e = kMp4Threads - 1 - tid;
    if (e < ne) {
      const int64_t p = s_box_p[1][e];
      const mp4::Box b = {true, mp4::kEmsg, s_box_hdr[1][e], s_box_size[1][e]};
      const mp4::Emsg m = mp4::emsg_parse(rd, p, b);
      v2l* row = reinterpret_cast<v2l*>(v.t.emsg + table_words(seg, max_emsg, mp4::kEmsgWords) + mp4::kEmsgWords * e);
      if (m.ok) {
        row[0] = v2l{p, b.size};
        row[1] = v2l{m.version, m.timescale};
        row[2] = v2l{m.time, m.is_delta};
        row[3] = v2l{m.duration, m.id};
        row[4] = v2l{m.data_off, m.data_len};
        row[5] = v2l{m.is_id3, 0};
      } else {
        atomicOr(&s_status, static_cast<int>(mp4::kBadBox));
#pragma unroll
        for (int i = 0; i < mp4::kEmsgWords / 2; ++i) row[i] = v2l{-1, -1};
      }
    }
  }
  for (int i = ne * (mp4::kEmsgWords / 2) + tid; i < max_emsg * (mp4::kEmsgWords / 2); i += kMp4Threads)
    reinterpret_cast<v2l*>(v.t.emsg + table_words(seg, max_emsg, mp4::kEmsgWords))[i] = v2l{-1, -1};
  const int inc = static_cast<int>(wave_scan_dpp(static_cast<uint32_t>(my_runs)));
  const WgPrefix<int> rp = wg_exclusive_prefix<kMp4Waves>(inc, my_runs, s_wave);
  const int n_run = rp.total, nr = n_run < max_run ? n_run : max_run;

  // ---- c. the same lanes walk again and record their runs in order; a row's kRnStartSample and
  // kRnTimeSample hold has_start and has_tfdt until step d settles the anchors
  if (moof_lane && my_runs > 0 && rp.before < max_run) {
    const int base = rp.before, moof = tid;
    mp4::moof_walk(rd, mp, mb, tracks, n, [&](int64_t j, const mp4::Run& r) {
      const int64_t g = base + j;
      if (g >= max_run) return;
      long long* row = s_run[g];
      row[mp4::kRnTrack] = r.track;
      row[mp4::kRnMoof] = moof;
      row[mp4::kRnFirst] = 0;
      row[mp4::kRnCount] = r.count;
      row[mp4::kRnEntries] = r.entries;
      row[mp4::kRnFlags] = r.flags;
      row[mp4::kRnTrafRun] = r.traf_run;
      row[mp4::kRnDefDuration] = r.def_duration;
      row[mp4::kRnDefSize] = r.def_size;
      row[mp4::kRnDefFlags] = r.def_flags;
      row[mp4::kRnFirstFlags] = r.first_flags;
      row[mp4::kRnStart] = r.start;
      row[mp4::kRnStartSample] = r.has_start ? 1 : 0;
      row[mp4::kRnTime] = r.tfdt;
      row[mp4::kRnTimeSample] = r.has_tfdt ? 1 : 0;
      row[mp4::kRnSpare] = 0;
    });
  }
  __syncthreads();

  // ---- d. a lane per run: its first sample among its track's, and its two anchors
  const bool run_lane = tid < nr;
  const int track = run_lane ? static_cast<int>(s_run[tid][mp4::kRnTrack]) : -1;
  const long long count = run_lane ? s_run[tid][mp4::kRnCount] : 0;
  const long long own0 = track == 0 ? count : 0, own1 = track == 1 ? count : 0;
  const WgPrefix<long long> f0 = wg_exclusive_prefix<kMp4Waves>(wave_scan64(own0), own0, s_wave0);
  const WgPrefix<long long> f1 = wg_exclusive_prefix<kMp4Waves>(wave_scan64(own1), own1, s_wave1);
  const long long first = track == 0 ? f0.before : f1.before;
  s_first[tid] = first;
  __syncthreads();
  long long start = 0, start_sample = 0, time = 0, time_sample = 0;
  if (run_lane) {
    auto run = [&](int64_t k) {
      const long long* row = s_run[k];
      mp4::Run r = {};
      r.track = static_cast<int>(row[mp4::kRnTrack]);
      r.traf_run = row[mp4::kRnTrafRun];
      r.has_start = row[mp4::kRnStartSample] != 0;
      r.has_tfdt = row[mp4::kRnTimeSample] != 0;
      return r;
    };
    const int64_t sa = mp4::start_anchor(run, tid), ta = mp4::time_anchor(run, tid);
    start = s_run[sa][mp4::kRnStart];
    start_sample = s_first[sa];
    time = ta >= 0 ? s_run[ta][mp4::kRnTime] : 0;
    time_sample = ta >= 0 ? s_first[ta] : 0;
  }
  __syncthreads();  // every lane has read the has_start / has_tfdt words
  if (run_lane) {
    long long* row = s_run[tid];
    row[mp4::kRnFirst] = first;
    row[mp4::kRnStart] = start;
    row[mp4::kRnStartSample] = start_sample;
    row[mp4::kRnTime] = time;
    row[mp4::kRnTimeSample] = time_sample;
  }
  __syncthreads();
  v2l* out = reinterpret_cast<v2l*>(v.t.runs + table_words(seg, max_run, mp4::kRunWords));
  const v2l* rows = reinterpret_cast<const v2l*>(&s_run[0][0]);
  for (int i = tid; i < max_run * (mp4::kRunWords / 2); i += kMp4Threads)
    out[i] = i < nr * (mp4::kRunWords / 2) ? rows[i] : v2l{-1, -1};

  if (tid == 0) {
    int64_t* mi = v.t.minfo + static_cast<int64_t>(seg) * mp4::kMinfoWords;
    int64_t status = s_top[0] | s_status;
    if (n_moof > max_moof) status |= mp4::kMoofOverflow;
    if (n_emsg > max_emsg) status |= mp4::kEmsgOverflow;
    if (n_run > max_run) status |= mp4::kRunOverflow;
    mi[mp4::kMStatus] = status;
    mi[mp4::kMNumMoof] = n_moof;
    mi[mp4::kMFirstSequence] = s_seq;
    mi[mp4::kMNumRun] = n_run;
    mi[mp4::kMNumOtherTraf] = s_other;
    mi[mp4::kMNumEmsg] = n_emsg;
  }
}

__global__ __launch_bounds__(kMp4Threads) void mp4_samples_kernel(Mp4View v) {
  __shared__ long long s_lfirst[mp4::kTracks][mp4::kMaxBoxRows];  // a track's runs: their first samples ...
  __shared__ long long s_at_size[mp4::kTracks][mp4::kMaxBoxRows], s_at_time[mp4::kTracks][mp4::kMaxBoxRows];  // ... and the sums there
  __shared__ long long s_excl_size[kMp4Threads], s_excl_time[kMp4Threads];
  __shared__ long long s_wave0[kMp4Waves], s_wave1[kMp4Waves];
  __shared__ long long s_total[mp4::kTracks], s_minmax[2], s_ends[mp4::kTracks][2];
  __shared__ int s_list[mp4::kTracks][mp4::kMaxBoxRows];  // ... and their rows
  __shared__ int s_wave[kMp4Waves], s_wave_b[kMp4Waves];
  __shared__ int s_status, s_sync;
  const int seg = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
  const int n = mp4_segment_bytes(v, seg);
  const int64_t max_pes = v.lim.max_pes;
  const int max_run = static_cast<int>(v.lim.max_run);
  SegReader rd = mp4_reader(v, seg, n);
  int64_t* mi = v.t.minfo + static_cast<int64_t>(seg) * mp4::kMinfoWords;
  const int64_t* runs = v.t.runs + table_words(seg, max_run, mp4::kRunWords);
  const int nr = static_cast<int>(clamp(mi[mp4::kMNumRun], 0, max_run));
  if (tid == 0) s_status = 0;
  if (tid < mp4::kTracks) {
    s_total[tid] = 0;
    s_ends[tid][0] = s_ends[tid][1] = -1;
  }

  // ---- a. the runs of each track, compacted in order
  const bool run_lane = tid < nr;
  const int track = run_lane ? static_cast<int>(runs[tid * mp4::kRunWords + mp4::kRnTrack]) : -1;
  const long long r_first = run_lane ? runs[tid * mp4::kRunWords + mp4::kRnFirst] : 0;
  const long long r_count = run_lane ? runs[tid * mp4::kRunWords + mp4::kRnCount] : 0;
  const int is0 = track == 0, is1 = track == 1;
  const int inc0 = __popcll(__ballot(is0) & (~0ull >> (63 - lane))), inc1 = __popcll(__ballot(is1) & (~0ull >> (63 - lane)));
  const WgPrefix<int> k0 = wg_exclusive_prefix<kMp4Waves>(inc0, is0, s_wave);
  const WgPrefix<int> k1 = wg_exclusive_prefix<kMp4Waves>(inc1, is1, s_wave_b);
  const int K[mp4::kTracks] = {k0.total, k1.total};
  if (is0 || is1) {
    const int pos = is0 ? k0.before : k1.before;
    s_lfirst[track][pos] = r_first;
    s_list[track][pos] = tid;
    if (pos == K[track] - 1) s_total[track] = r_first + r_count;
  }
  __syncthreads();

  const int64_t* tracks = v.tracks + seg * mp4::kTracks * mp4::kTrackWords;
  int64_t n_samples[mp4::kTracks];
  for (int t = 0; t < mp4::kTracks; ++t) {
    const long long N = s_total[t];
    n_samples[t] = N;
    const int Kt = K[t];
    const int64_t rec = N < max_pes ? N : max_pes;
    int64_t* pes = v.t.pes + ts::pes_words(seg, max_pes) + table_words(t, max_pes, ts::kPesWords);
    int32_t* ms = v.t.msamples + table_words(seg, mp4::kTracks * max_pes, mp4::kMsampleWords) +
                  table_words(t, max_pes, mp4::kMsampleWords);
    if (tid == 0) {
      s_minmax[0] = 0x7fffffffffffffffll;
      s_minmax[1] = -0x7fffffffffffffffll - 1;
      s_sync = 0x7fffffff;
    }
    __syncthreads();

    // ---- b. rounds of 256 samples with a carry
    long long carry_size = 0, carry_time = 0;
    int flags_or = 0;
    for (long long base = 0; base < N; base += kMp4Threads) {
      const long long i = base + tid;
      const bool valid = i < N;
      mp4::Sample s = {0, 0, 0, 0};
      const int64_t* row = runs;
      if (valid) {
        const int k = last_le_lds(s_lfirst[t], Kt, i);
        row = runs + static_cast<int64_t>(s_list[t][k]) * mp4::kRunWords;
        s = mp4::sample_at(rd, row[mp4::kRnEntries], static_cast<uint32_t>(row[mp4::kRnFlags]), i - s_lfirst[t][k],
                           static_cast<uint32_t>(row[mp4::kRnDefDuration]), static_cast<uint32_t>(row[mp4::kRnDefSize]),
                           static_cast<uint32_t>(row[mp4::kRnDefFlags]), row[mp4::kRnFirstFlags]);
      }
      const long long own_size = valid ? s.size : 0, own_time = valid ? s.duration : 0;
      const WgPrefix<long long> ps = wg_exclusive_prefix<kMp4Waves>(wave_scan64(own_size), own_size, s_wave0);
      const WgPrefix<long long> pt = wg_exclusive_prefix<kMp4Waves>(wave_scan64(own_time), own_time, s_wave1);
      const long long sizes = carry_size + ps.before, times = carry_time + pt.before;
      s_excl_size[tid] = sizes;
      s_excl_time[tid] = times;
      __syncthreads();
      // the runs whose first sample lies in this round keep the two sums there
      if (tid < Kt) {
        const long long f = s_lfirst[t][tid];
        if (f >= base && f < base + kMp4Threads) {
          s_at_size[t][tid] = s_excl_size[f - base];
          s_at_time[t][tid] = s_excl_time[f - base];
        }
      }
      __syncthreads();
      if (valid && i < max_pes) {
        // any run that starts at the anchor's sample holds the same sums
        const long long s0 = s_at_size[t][last_le_lds(s_lfirst[t], Kt, row[mp4::kRnStartSample])];
        const long long d0 = s_at_time[t][last_le_lds(s_lfirst[t], Kt, row[mp4::kRnTimeSample])];
        const mp4::Placed pl = mp4::place_sample(mp4::wrap_add(row[mp4::kRnStart], mp4::wrap_sub(sizes, s0)), s.size, n);
        const int64_t dts = mp4::wrap_add(row[mp4::kRnTime], mp4::wrap_sub(times, d0));
        const int64_t pts = mp4::wrap_add(dts, s.cts);
        const es::Delta32 d = mp4::duration32(s.duration);
        if (pl.clipped) flags_or |= static_cast<int>(mp4::kSampleOutOfRange);
        if (!d.fits) flags_or |= static_cast<int>(mp4::kBadTimestamps);
        pes[ts::kPesWords * i + ts::kPesEsOffset] = pl.off;
        pes[ts::kPesWords * i + ts::kPesPts] = pts;
        pes[ts::kPesWords * i + ts::kPesDts] = dts;
        reinterpret_cast<v4i*>(ms)[i] =
            v4i{static_cast<int>(pl.size), d.v, s.cts, static_cast<int>(s.flags)};
        __hip_atomic_fetch_min(&s_minmax[0], static_cast<long long>(pts), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        __hip_atomic_fetch_max(&s_minmax[1], static_cast<long long>(pts), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (!(s.flags & mp4::kSampleNonSyncBit)) atomicMin(&s_sync, static_cast<int>(i));
        if (i == 0) s_ends[t][0] = pts;
        if (i == rec - 1) s_ends[t][1] = pts;
      }
      carry_size += ps.total;
      carry_time += pt.total;
      __syncthreads();  // s_wave*, s_excl_* are free again
    }
    if (flags_or) atomicOr(&s_status, flags_or);

    // ---- c. the rows beyond the recorded samples, and the track's words of minfo
    for (int64_t w = rec * ts::kPesWords + tid; w < max_pes * ts::kPesWords; w += kMp4Threads) pes[w] = -1;
    for (int64_t r = rec + tid; r < max_pes; r += kMp4Threads) reinterpret_cast<v4i*>(ms)[r] = v4i{-1, -1, -1, -1};
    __syncthreads();
    if (tid == 0) {
      int64_t* mt = mi + mp4::kMTrack0 + mp4::kMTrackWords * t;
      mt[mp4::kMtNumSamples] = N;
      mt[mp4::kMtBaseTime] = Kt > 0 ? runs[static_cast<int64_t>(s_list[t][0]) * mp4::kRunWords + mp4::kRnTime] : -1;
      mt[mp4::kMtDuration] = carry_time;
      mt[mp4::kMtMinPts] = rec > 0 ? s_minmax[0] : -1;
      mt[mp4::kMtMaxPts] = rec > 0 ? s_minmax[1] : -1;
      mt[mp4::kMtFirstSync] = s_sync == 0x7fffffff ? -1 : s_sync;
      if (N > max_pes) s_status |= static_cast<int>(mp4::kSampleOverflow);
    }
    __syncthreads();
  }

  // ---- d. the id3 class has no rows; the demux row: the whole segment is the video ES
  int64_t* pes2 = v.t.pes + ts::pes_words(seg, max_pes) + table_words(2, max_pes, ts::kPesWords);
  for (int64_t w = tid; w < max_pes * ts::kPesWords; w += kMp4Threads) pes2[w] = -1;
  if (tid == 0) {
    const int64_t* at = tracks + mp4::kTrackWords;
    int64_t* info = v.t.info + static_cast<int64_t>(seg) * ts::kInfoWords;
    for (int w = 0; w < ts::kInfoWords; ++w) info[w] = 0;
    info[ts::kPmtPid] = -1;
    info[ts::kVideoPid] = tracks[mp4::kTkId] > 0 ? tracks[mp4::kTkId] : -1;
    info[ts::kAudioPid] = at[mp4::kTkId] > 0 ? at[mp4::kTkId] : -1;
    info[ts::kId3Pid] = -1;
    info[ts::kVideoBytes] = n;
    info[ts::kNumVideoPes] = n_samples[0];
    info[ts::kVideoType] = mp4::video_indexed(tracks) ? tracks[mp4::kTkCodecType] : 0;
    info[ts::kAudioType] = at[mp4::kTkId] > 0 ? at[mp4::kTkCodecType] : 0;
    info[ts::kPayloadBytes] = n;
    for (int c = 0; c < ts::kClasses; ++c) {
      info[ts::kFirstPts + c] = c < mp4::kTracks ? s_ends[c][0] : -1;
      info[ts::kLastPts + c] = c < mp4::kTracks ? s_ends[c][1] : -1;
    }
    info[ts::kAudioEsOffset] = n;
    mi[mp4::kMStatus] |= s_status;
  }
}

__global__ __launch_bounds__(kMp4Threads) void mp4_nal_kernel(Mp4View v) {
  __shared__ long long s_wave0[kMp4Waves];
  __shared__ int s_keys, s_first_key, s_error;
  const int seg = blockIdx.x, tid = threadIdx.x;
  const int n = mp4_segment_bytes(v, seg);
  const int64_t max_pes = v.lim.max_pes, max_nal = v.lim.max_nal;
  SegReader rd = mp4_reader(v, seg, n);
  const int64_t* tracks = v.tracks + seg * mp4::kTracks * mp4::kTrackWords;
  int64_t* mi = v.t.minfo + static_cast<int64_t>(seg) * mp4::kMinfoWords;
  const bool indexed = mp4::video_indexed(tracks);
  const bool hevc = es::is_hevc(tracks[mp4::kTkCodecType]);
  const int L = static_cast<int>(tracks[mp4::kTkNalLengthSize]);
  const int64_t m = indexed ? clamp(mi[mp4::kMTrack0 + mp4::kMtNumSamples], 0, max_pes) : 0;
  const int64_t* pes = v.t.pes + ts::pes_words(seg, max_pes);
  const v4i* ms = reinterpret_cast<const v4i*>(v.t.msamples + table_words(seg, mp4::kTracks * max_pes, mp4::kMsampleWords));
  v4i* nal = reinterpret_cast<v4i*>(v.t.ix.nal + table_words(seg, max_nal, es::kNalWords));
  v4i* au = reinterpret_cast<v4i*>(v.t.ix.au + table_words(seg, max_pes, es::kAuWords));
  if (tid == 0) {
    s_keys = 0;
    s_first_key = 0x7fffffff;
    s_error = 0;
  }
  __syncthreads();

  // ---- a. a lane per recorded video sample counts its NAL units, a scan ranks them, the lane
  // walks again and writes their rows and its own
  long long carry = 0;
  for (int64_t ab = 0; ab < m; ab += kMp4Threads) {
    const int64_t a = ab + tid;
    const bool valid = a < m;
    int64_t off = 0, end = 0;
    long long count = 0;
    if (valid) {
      off = clamp(pes[ts::kPesWords * a + ts::kPesEsOffset], 0, n);
      end = off + clamp(ms[a][mp4::kMsSize], 0, n - off);
      int64_t q = off, s = 0, len = 0;
      int step;
      while ((step = mp4::nal_step(rd, q, end, L, s, len)) == 1) {
        ++count;
        q = s + len;
      }
      if (step == 2 || q != end) s_error = 1;
    }
    const WgPrefix<long long> p = wg_exclusive_prefix<kMp4Waves>(wave_scan64(count), count, s_wave0);
    if (valid) {
      const long long rank = carry + p.before;
      int64_t q = off, s = 0, len = 0;
      int kept = 0, flags = 0;
      long long k = rank;
      while (k < max_nal && mp4::nal_step(rd, q, end, L, s, len) == 1) {
        const int type = len ? es::nal_type(hevc, rd.u8(s)) : -1;
        nal[k] = v4i{static_cast<int>(s), static_cast<int>(len), type, static_cast<int>(a)};
        flags |= es::nal_flags(hevc, type);
        ++kept;
        ++k;
        q = s + len;
      }
      au[a] = v4i{kept ? static_cast<int>(rank) : -1, kept, flags, static_cast<int>(end - off)};
      if (flags & es::kAuKeyframe) {
        atomicAdd(&s_keys, 1);
        atomicMin(&s_first_key, static_cast<int>(a));
      }
    }
    carry += p.total;
    __syncthreads();  // s_wave0 is free again
  }

  // ---- b. the rows beyond, 16 bytes per store where a row is one; sinfo
  const int64_t nn = carry < max_nal ? carry : max_nal;
  for (int64_t k = nn + tid; k < max_nal; k += kMp4Threads) nal[k] = v4i{-1, -1, -1, -1};
  for (int64_t a = m + tid; a < max_pes; a += kMp4Threads) au[a] = v4i{-1, -1, -1, -1};
  long long* af = reinterpret_cast<long long*>(v.t.ix.aframes + table_words(seg, max_pes, es::kApesWords));
  static_assert(es::kApesWords == 2, "an aframes row is one 8-byte store");
  for (int64_t a = tid; a < max_pes; a += kMp4Threads) af[a] = -1;
  if (tid == 0) {
    int64_t* si = v.t.ix.sinfo + static_cast<int64_t>(seg) * es::kSinfoWords;
    si[es::kStatus] = !indexed ? es::kUnsupportedVideo : carry > max_nal ? es::kNalOverflow : 0;
    si[es::kNumNal] = carry;
    si[es::kNumAu] = m;
    si[es::kNumKeyframeAus] = s_keys;
    si[es::kFirstKeyframeAu] = s_first_key == 0x7fffffff ? -1 : s_first_key;
    si[es::kNumAdtsFrames] = 0;
    si[es::kAudioSampleRate] = 0;
    si[es::kAudioChannels] = 0;
    if (s_error) mi[mp4::kMStatus] |= mp4::kNalError;
  }
}

hipError_t launch_mp4_demux(const Mp4DemuxArgs& a) {
  if (a.nseg <= 0) return hipSuccess;
  if (a.lim.max_pes <= 0 || a.lim.max_pes > 0x7fffffff || a.lim.max_nal <= 0 || a.lim.max_nal > 0x7fffffff ||
      !mp4::max_rows_ok(a.lim.max_moof) || !mp4::max_rows_ok(a.lim.max_run) || !mp4::max_rows_ok(a.lim.max_emsg))
    return hipErrorInvalidValue;
  const Mp4View v = {a.buf, a.buf_numel, a.off, a.len, a.cap, a.tracks, a.lim, a.t};
  hipLaunchKernelGGL(mp4_boxes_kernel, dim3(a.nseg), dim3(kMp4Threads), 0, a.stream, v);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(mp4_samples_kernel, dim3(a.nseg), dim3(kMp4Threads), 0, a.stream, v);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(mp4_nal_kernel, dim3(a.nseg), dim3(kMp4Threads), 0, a.stream, v);
  return hipGetLastError();
}

}  // namespace dev
}  // namespace hlsp2p
