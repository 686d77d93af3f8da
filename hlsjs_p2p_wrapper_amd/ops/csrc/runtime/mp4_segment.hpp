// The sequential fragmented-MP4 demux of one segment over any reader (docs/FMP4DEMUX.md): one pass
// per stage (boxes, runs, samples, NAL units).  runtime/mp4.cpp runs it over a reader with a range
// test; tests/native/mp4_main.cpp also over one without, under a sanitizer.  The box header, the
// moof / traf walk, the trun entry, the sample placement, the NAL step and the emsg rules are
// shared/grammar.hpp (namespace mp4), the same functions kernels/mp4_demux.hip calls.
#pragma once
#include <algorithm>
#include <vector>

#include "mp4.hpp"

namespace hlsp2p {
namespace mp4 {

struct MoofAt {
  int64_t p;
  Box b;
};
struct RunAt {
  Run r;
  int64_t moof, first;
};

// rd.u8(p) / rd.be32(p): byte p of the segment's n bytes; asked only for bytes of [0, n)
template <class Reader>
void demux_segment_with(Reader rd, int64_t n, const int64_t* tracks, const Limits& lim, const Tables& out) {
  const int64_t max_pes = lim.max_pes, max_nal = lim.max_nal;
  std::fill(out.minfo, out.minfo + kMinfoWords, int64_t(0));
  std::fill(out.msamples, out.msamples + table_words(1, kTracks * max_pes, kMsampleWords), -1);
  std::fill(out.runs, out.runs + table_words(1, lim.max_run, kRunWords), int64_t(-1));
  std::fill(out.emsg, out.emsg + table_words(1, lim.max_emsg, kEmsgWords), int64_t(-1));
  std::fill(out.info, out.info + ts::kInfoWords, int64_t(0));
  std::fill(out.pes, out.pes + ts::pes_words(1, max_pes), int64_t(-1));
  std::fill(out.ix.nal, out.ix.nal + table_words(1, max_nal, es::kNalWords), -1);
  std::fill(out.ix.au, out.ix.au + table_words(1, max_pes, es::kAuWords), -1);
  std::fill(out.ix.aframes, out.ix.aframes + table_words(1, max_pes, es::kApesWords), -1);
  std::fill(out.ix.sinfo, out.ix.sinfo + es::kSinfoWords, int64_t(0));
  n = std::max<int64_t>(n, 0);
  int64_t status = 0;

  // ---- the top level: moof and emsg boxes
  std::vector<MoofAt> moofs;
  const TopOut top = top_walk(
      rd, n,
      [&](int64_t k, int64_t p, const Box& b) {
        if (k < lim.max_moof) moofs.push_back({p, b});
      },
      [&](int64_t k, int64_t p, const Box& b) {
        if (k >= lim.max_emsg) return;
        const Emsg e = emsg_parse(rd, p, b);
        if (!e.ok) {
          status |= kBadBox;
          return;
        }
        int64_t* row = out.emsg + kEmsgWords * k;
        row[kEmOffset] = p;
        row[kEmSize] = b.size;
        row[kEmVersion] = e.version;
        row[kEmTimescale] = e.timescale;
        row[kEmTime] = e.time;
        row[kEmTimeIsDelta] = e.is_delta;
        row[kEmDuration] = e.duration;
        row[kEmId] = e.id;
        row[kEmDataOffset] = e.data_off;
        row[kEmDataLength] = e.data_len;
        row[kEmIsId3] = e.is_id3;
        row[kEmSpare] = 0;
      });
  status |= top.status;
  if (top.n_moof > lim.max_moof) status |= kMoofOverflow;
  if (top.n_emsg > lim.max_emsg) status |= kEmsgOverflow;

  // ---- inside the moofs: the runs of the configured tracks
  std::vector<RunAt> runs;
  int64_t n_run = 0, n_other = 0, first_seq = -1;
  for (size_t k = 0; k < moofs.size(); ++k) {
    const MoofOut o = moof_walk(rd, moofs[k].p, moofs[k].b, tracks, n, [&](int64_t, const Run& r) {
      if (n_run++ < lim.max_run) runs.push_back({r, static_cast<int64_t>(k), 0});
    });
    status |= o.status;
    n_other += o.n_other;
    if (k == 0) first_seq = o.seq;
  }
  if (n_run > lim.max_run) status |= kRunOverflow;
  const int64_t R = static_cast<int64_t>(runs.size());
  int64_t total[kTracks] = {0, 0};
  for (RunAt& a : runs) {
    a.first = total[a.r.track];
    total[a.r.track] += a.r.count;
  }
  auto run_at = [&](int64_t k) { return runs[static_cast<size_t>(k)].r; };
  for (int64_t r = 0; r < R; ++r) {
    const RunAt& a = runs[static_cast<size_t>(r)];
    const RunAt& sa = runs[static_cast<size_t>(start_anchor(run_at, r))];
    const int64_t ta = time_anchor(run_at, r);
    int64_t* row = out.runs + kRunWords * r;
    row[kRnTrack] = a.r.track;
    row[kRnMoof] = a.moof;
    row[kRnFirst] = a.first;
    row[kRnCount] = a.r.count;
    row[kRnEntries] = a.r.entries;
    row[kRnFlags] = a.r.flags;
    row[kRnTrafRun] = a.r.traf_run;
    row[kRnDefDuration] = a.r.def_duration;
    row[kRnDefSize] = a.r.def_size;
    row[kRnDefFlags] = a.r.def_flags;
    row[kRnFirstFlags] = a.r.first_flags;
    row[kRnStart] = sa.r.start;
    row[kRnStartSample] = sa.first;
    row[kRnTime] = ta >= 0 ? runs[static_cast<size_t>(ta)].r.tfdt : 0;
    row[kRnTimeSample] = ta >= 0 ? runs[static_cast<size_t>(ta)].first : 0;
    row[kRnSpare] = 0;
  }

  // ---- the samples of each track, in run and entry order
  std::vector<int64_t> size_at(static_cast<size_t>(R), 0), time_at(static_cast<size_t>(R), 0);
  int64_t first_pts[kTracks] = {-1, -1}, last_pts[kTracks] = {-1, -1};
  for (int t = 0; t < kTracks; ++t) {
    int64_t* mt = out.minfo + kMTrack0 + kMTrackWords * t;
    int64_t* pes = out.pes + table_words(t, max_pes, ts::kPesWords);
    int32_t* ms = out.msamples + table_words(t, max_pes, kMsampleWords);
    int64_t sizes = 0, durations = 0, i = 0, min_pts = -1, max_pts = -1, first_sync = -1, base_time = -1;
    bool seen_run = false;
    for (int64_t r = 0; r < R; ++r) {
      const RunAt& a = runs[static_cast<size_t>(r)];
      if (a.r.track != t) continue;
      size_at[static_cast<size_t>(r)] = sizes;
      time_at[static_cast<size_t>(r)] = durations;
      const int64_t* row = out.runs + kRunWords * r;
      // the sums at the first sample of the two anchor runs: rows of this track at or in front of r
      const int64_t s0 = size_at[static_cast<size_t>(start_anchor(run_at, r))];
      const int64_t ta = time_anchor(run_at, r);
      const int64_t d0 = ta >= 0 ? time_at[static_cast<size_t>(ta)] : 0;
      if (!seen_run) base_time = row[kRnTime];  // the track's first run: its traf's decode time
      seen_run = true;
      for (int64_t j = 0; j < a.r.count; ++j, ++i) {
        const Sample s = sample_at(rd, a.r.entries, a.r.flags, j, a.r.def_duration, a.r.def_size, a.r.def_flags,
                                   a.r.first_flags);
        if (i < max_pes) {
          const Placed pl = place_sample(wrap_add(row[kRnStart], wrap_sub(sizes, s0)), s.size, n);
          const int64_t dts = wrap_add(row[kRnTime], wrap_sub(durations, d0));
          const int64_t pts = wrap_add(dts, s.cts);
          if (pl.clipped) status |= kSampleOutOfRange;
          const es::Delta32 d = duration32(s.duration);
          if (!d.fits) status |= kBadTimestamps;
          pes[ts::kPesWords * i + ts::kPesEsOffset] = pl.off;
          pes[ts::kPesWords * i + ts::kPesPts] = pts;
          pes[ts::kPesWords * i + ts::kPesDts] = dts;
          int32_t* m = ms + kMsampleWords * i;
          m[kMsSize] = static_cast<int32_t>(pl.size);
          m[kMsDuration] = d.v;
          m[kMsCts] = s.cts;
          m[kMsFlags] = static_cast<int32_t>(s.flags);
          min_pts = i == 0 ? pts : std::min(min_pts, pts);
          max_pts = i == 0 ? pts : std::max(max_pts, pts);
          if (first_sync < 0 && !(s.flags & kSampleNonSyncBit)) first_sync = i;
          if (i == 0) first_pts[t] = pts;
          last_pts[t] = pts;
        }
        sizes = wrap_add(sizes, s.size);
        durations = wrap_add(durations, s.duration);
      }
    }
    if (i > max_pes) status |= kSampleOverflow;
    mt[kMtNumSamples] = i;
    mt[kMtBaseTime] = base_time;
    mt[kMtDuration] = durations;
    mt[kMtMinPts] = min_pts;
    mt[kMtMaxPts] = max_pts;
    mt[kMtFirstSync] = first_sync;
  }

  // ---- the demux row: the whole segment is the video ES, there is no audio ES
  const bool indexed = video_indexed(tracks);
  const int64_t* at = tracks + kTrackWords;
  int64_t* info = out.info;
  info[ts::kPmtPid] = -1;
  info[ts::kVideoPid] = tracks[kTkId] > 0 ? tracks[kTkId] : -1;
  info[ts::kAudioPid] = at[kTkId] > 0 ? at[kTkId] : -1;
  info[ts::kId3Pid] = -1;
  info[ts::kVideoBytes] = n;
  info[ts::kNumVideoPes] = out.minfo[kMTrack0 + kMtNumSamples];
  info[ts::kVideoType] = indexed ? tracks[kTkCodecType] : 0;
  info[ts::kAudioType] = at[kTkId] > 0 ? at[kTkCodecType] : 0;
  info[ts::kPayloadBytes] = n;
  for (int c = 0; c < ts::kClasses; ++c) {
    info[ts::kFirstPts + c] = c < kTracks ? first_pts[c] : -1;
    info[ts::kLastPts + c] = c < kTracks ? last_pts[c] : -1;
  }
  info[ts::kAudioEsOffset] = n;

  // ---- the NAL units of the recorded video samples
  int64_t* sinfo = out.ix.sinfo;
  sinfo[es::kFirstKeyframeAu] = -1;
  if (!indexed) {
    sinfo[es::kStatus] = es::kUnsupportedVideo;
  } else {
    const bool hevc = es::is_hevc(tracks[kTkCodecType]);
    const int L = static_cast<int>(tracks[kTkNalLengthSize]);
    const int64_t m = std::min(out.minfo[kMTrack0 + kMtNumSamples], max_pes);
    int64_t n_nal = 0, n_key = 0, first_key = -1;
    for (int64_t a = 0; a < m; ++a) {
      const int64_t off = out.pes[ts::kPesWords * a + ts::kPesEsOffset];
      const int64_t end = off + out.msamples[kMsampleWords * a + kMsSize];
      int64_t q = off, s = 0, len = 0;
      int32_t first = -1, count = 0, flags = 0;
      int step;
      while ((step = nal_step(rd, q, end, L, s, len)) == 1) {
        if (n_nal < max_nal) {
          const int type = len ? es::nal_type(hevc, rd.u8(s)) : -1;
          int32_t* row = out.ix.nal + es::kNalWords * n_nal;
          row[es::kNalOffset] = static_cast<int32_t>(s);
          row[es::kNalLength] = static_cast<int32_t>(len);
          row[es::kNalType] = type;
          row[es::kNalAu] = static_cast<int32_t>(a);
          if (count++ == 0) first = static_cast<int32_t>(n_nal);
          flags |= es::nal_flags(hevc, type);
        }
        ++n_nal;
        q = s + len;
      }
      if (step == 2 || q != end) status |= kNalError;
      int32_t* row = out.ix.au + es::kAuWords * a;
      row[es::kAuFirstNal] = first;
      row[es::kAuNalCount] = count;
      row[es::kAuFlags] = flags;
      row[es::kAuSize] = out.msamples[kMsampleWords * a + kMsSize];
      if (flags & es::kAuKeyframe) {
        if (n_key++ == 0) first_key = a;
      }
    }
    sinfo[es::kStatus] = n_nal > max_nal ? es::kNalOverflow : 0;
    sinfo[es::kNumNal] = n_nal;
    sinfo[es::kNumAu] = m;
    sinfo[es::kNumKeyframeAus] = n_key;
    sinfo[es::kFirstKeyframeAu] = first_key;
  }

  out.minfo[kMStatus] = status;
  out.minfo[kMNumMoof] = top.n_moof;
  out.minfo[kMFirstSequence] = first_seq;
  out.minfo[kMNumRun] = n_run;
  out.minfo[kMNumOtherTraf] = n_other;
  out.minfo[kMNumEmsg] = top.n_emsg;
}

}  // namespace mp4
}  // namespace hlsp2p
