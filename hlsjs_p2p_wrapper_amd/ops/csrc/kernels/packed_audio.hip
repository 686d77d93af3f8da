// Demux of packed-audio segments: ID3v2 tags in front of raw ADTS frames (docs/PACKEDAUDIO.md) —
// CDNA4 / gfx950.
//
// Input: the segments where the decrypt left them, only read.
// Output per segment, identical to the host implementation runtime/packedaudio.cpp packed_segment:
//   info / pes in the layout of ts_demux.hip, nal (one row) / au / aframes / sinfo in that of
//   es_index.hip, painfo: int64[seg][kPainfoWords]
//
// One launch, one 256-thread workgroup per segment; no workgroup waits for another.
//   a. Lane 0 walks the leading tags and the frames of the tag that may hold the timestamp through
//      a buffer resource that ends with the segment (SegReader of mp4_dev.h): a few dependent
//      16-byte loads for a real segment.
//   b. The frame chain is serial: each header gives the next position.  All 256 lanes stage a tile
//      of kPackedTile bytes into LDS, 16 bytes per load through the same buffer resource (a byte
//      beyond the segment's last dword reads 0), lane 0 walks the frames inside the tile with
//      es::adts_frame_at over the staged bytes (a header's 8 bytes in one LDS round trip) and leaves
//      each group's first byte in an LDS list of max_pes + 1 entries.  When the next 7-byte header
//      would pass the tile's end the next tile starts at q & ~15: a frame is at most 8,191 bytes,
//      so every tile makes progress.
//      (kStaged = false walks the frames through the buffer resource instead: a 16-byte load per
//      frame, each a round trip to memory.  tools/kernel_bench.py measures both.)
//   c. A lane per row writes pes, au and aframes with their -1 fill; 24 + 8 + 8 lanes write info,
//      sinfo and painfo from the shared summary.
// Plain vector stores only.  All byte rules are shared/grammar.hpp (namespace es), the same
// functions runtime/packedaudio.cpp calls.
#include "launch.h"
#include "mp4_dev.h"

namespace hlsp2p {
namespace dev {

constexpr int kPaThreads = 256;
constexpr int kPaLoads = es::kPackedTile / (16 * kPaThreads);  // 16-byte loads of a lane per tile
static_assert(es::kPackedTile % (16 * kPaThreads) == 0, "every lane stages the same number of 16-byte lines");
static_assert(es::kPackedTile >= 8191 + 16 + 7, "a tile holds a whole frame behind any start");
static_assert(es::kAuWords == 4 && es::kNalWords == 4 && es::kApesWords == 2, "16- and 8-byte rows");

// Passed by value as the first kernel parameter.
struct PackedView {
  const uint8_t* buf;
  int64_t buf_numel;
  const int64_t *off, *len, *cap;
  int64_t max_pes;
  es::PackedTables t;
};

template <bool kStaged>
__global__ __launch_bounds__(kPaThreads) void packed_audio_kernel(PackedView v) {
  __shared__ __attribute__((aligned(16))) uint8_t s_tile[kStaged ? es::kPackedTile + 16 : 16];  // + a header read's spare dwords
  extern __shared__ int s_first[];  // max_pes + 1: the first byte of a group, of the one behind the last
  __shared__ es::PackedSummary s_sum;
  __shared__ int s_q, s_more;
  const int seg = blockIdx.x, tid = threadIdx.x;
  const int n = static_cast<int>(clamp(v.len[seg], 0, clamp(v.cap[seg], 0, 0x7fffffff)));
  const int max_pes = static_cast<int>(v.max_pes);
  SegReader rd = mp4_reader(v.buf, v.buf_numel, v.off[seg], n);

  // ---- a. the tags, one lane
  es::PackedTags tags = {0, 0, 0, -1};
  int q = 0, n_frames = 0, rate = 0, chans = 0;  // lane 0's walk
  if (tid == 0) {
    tags = es::packed_tags(rd, n);
    q = static_cast<int>(tags.T);
    s_q = q;
    s_more = !(tags.status & es::kPaBadId3);
  }
  __syncthreads();

  // ---- b. the frame chain
  auto take = [&](int b2, int b3, int len) {  // lane 0: the frame at q counts
    if (n_frames == 0) {
      rate = es::adts_rate((b2 >> 2) & 15);
      chans = es::adts_channels(b2, b3);
    }
    if ((n_frames % es::kPackedFramesPerPes) == 0) {
      const int k = n_frames / es::kPackedFramesPerPes;
      if (k <= max_pes) s_first[k] = q;
    }
    ++n_frames;
    q += len;
  };
  if constexpr (kStaged) {
    while (s_more) {
      const uint32_t base = static_cast<uint32_t>(s_q) & ~15u;
      v4u w[kPaLoads];
#pragma unroll
      for (int k = 0; k < kPaLoads; ++k)
        w[k] = __builtin_amdgcn_raw_buffer_load_b128(rd.rsrc, static_cast<int>(base + 16u * (tid + k * kPaThreads)), 0, 0);
#pragma unroll
      for (int k = 0; k < kPaLoads; ++k) reinterpret_cast<v4u*>(s_tile)[tid + k * kPaThreads] = w[k];
      __syncthreads();
      if (tid == 0) {
        const int64_t b = base, tile_end = b + es::kPackedTile;
        bool more = false;
        for (;;) {
          if (int64_t(q) + 7 > n) break;  // no header fits: adts_frame_at's first test, in front of the LDS read
          if (int64_t(q) + 7 > tile_end) {  // the next header passes the tile's end
            more = true;
            break;
          }
          // the header's 8 bytes in one LDS round trip: three aligned dwords, funnelled (a byte test
          // after the other would wait for LDS four times per frame)
          const uint32_t rel = static_cast<uint32_t>(q - b), sh = rel & 3;
          const uint32_t* wp = reinterpret_cast<const uint32_t*>(s_tile) + (rel >> 2);
          const uint32_t w0 = wp[0], w1 = wp[1], w2 = wp[2];
          const uint32_t lo = __builtin_amdgcn_alignbyte(w1, w0, sh), hi = __builtin_amdgcn_alignbyte(w2, w1, sh);
          uint8_t h[8];
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            h[i] = static_cast<uint8_t>(lo >> (8 * i));
            h[4 + i] = static_cast<uint8_t>(hi >> (8 * i));
          }
          const es::AdtsFrame f = es::adts_frame_at(h, 0, int64_t(n) - q);
          if (f.len == 0) break;
          take(h[2], h[3], f.len);
        }
        s_q = q;
        s_more = more;
      }
      __syncthreads();
    }
  } else {
    if (tid == 0 && s_more) {
      for (;;) {
        uint8_t h[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) h[i] = static_cast<uint8_t>(rd.u8(int64_t(q) + i));  // one 16-byte load
        const es::AdtsFrame f = es::adts_frame_at(h, 0, int64_t(n) - q);
        if (f.len == 0) break;
        take(h[2], h[3], f.len);
      }
    }
  }
  if (tid == 0) {
    const int64_t groups = es::packed_groups(n_frames);
    if (groups <= max_pes) s_first[groups] = q;
    s_sum = es::packed_summary(tags, n_frames, q, rate, chans, n, max_pes);
  }
  __syncthreads();

  // ---- c. the rows
  const es::PackedSummary s = s_sum;
  const int64_t groups = es::packed_groups(s.n_frames);
  const int rec = static_cast<int>(groups < max_pes ? groups : max_pes);
  int64_t* pes = v.t.pes + ts::pes_words(seg, max_pes);
  for (int r = tid; r < ts::kClasses * max_pes; r += kPaThreads) {
    const int cls = r / max_pes, k = r - cls * max_pes;
    int64_t off = -1, stamp = -1;
    if (cls == 1 && k < rec) {
      off = s_first[k] - s.T;
      stamp = es::packed_stamp(s.ts, k, s.rate);
    } else if (cls == 2 && k == 0 && s.T > 0) {
      off = 0;
      stamp = s.ts;
    }
    int64_t* row = pes + int64_t(ts::kPesWords) * r;
    row[ts::kPesEsOffset] = off;
    row[ts::kPesPts] = stamp;
    row[ts::kPesDts] = stamp;
  }
  v4i* au = reinterpret_cast<v4i*>(v.t.ix.au + table_words(seg, max_pes, es::kAuWords));
  int2* af = reinterpret_cast<int2*>(v.t.ix.aframes + table_words(seg, max_pes, es::kApesWords));
  for (int k = tid; k < max_pes; k += kPaThreads) {
    au[k] = v4i{-1, -1, -1, -1};
    int2 row = {-1, -1};
    if (k < rec) {
      const int64_t left = s.n_frames - int64_t(es::kPackedFramesPerPes) * k;
      row.x = static_cast<int>(left < es::kPackedFramesPerPes ? left : es::kPackedFramesPerPes);
      row.y = s_first[k + 1] - s_first[k];
    }
    af[k] = row;
  }
  if (tid == 0)
    reinterpret_cast<v4i*>(v.t.ix.nal + table_words(seg, es::kPackedNalRows, es::kNalWords))[0] = v4i{-1, -1, -1, -1};
  if (tid < ts::kInfoWords) v.t.info[int64_t(seg) * ts::kInfoWords + tid] = es::packed_info_word(tid, s, max_pes);
  const int t1 = tid - 64, t2 = tid - 128;
  if (t1 >= 0 && t1 < es::kSinfoWords) v.t.ix.sinfo[int64_t(seg) * es::kSinfoWords + t1] = es::packed_sinfo_word(t1, s);
  if (t2 >= 0 && t2 < es::kPainfoWords) v.t.painfo[int64_t(seg) * es::kPainfoWords + t2] = es::packed_painfo_word(t2, s);
}

int packed_audio_tile_bytes() { return es::kPackedTile; }

hipError_t launch_packed_audio(const PackedAudioArgs& a) {
  if (a.nseg <= 0) return hipSuccess;
  if (!es::packed_max_pes_ok(a.max_pes)) return hipErrorInvalidValue;
  const PackedView v = {a.buf, a.buf_numel, a.off, a.len, a.cap, a.max_pes, a.t};
  const size_t list = static_cast<size_t>(a.max_pes + 1) * sizeof(int);
  if (a.staged)
    hipLaunchKernelGGL(packed_audio_kernel<true>, dim3(a.nseg), dim3(kPaThreads), list, a.stream, v);
  else
    hipLaunchKernelGGL(packed_audio_kernel<false>, dim3(a.nseg), dim3(kPaThreads), list, a.stream, v);
  return hipGetLastError();
}

}  // namespace dev
}  // namespace hlsp2p
