// The device side of launch.h's EsBatch: the batch as every kernel behind the demux takes it, one
// segment of it, and the segment's ES as a buffer resource.  The bounds every such kernel relies
// on are set here: the cap clamped to int32, the row counts clamped to the tables, and a resource
// that ends with the ES tensor.
#pragma once
#include "common.h"
#include "grammar.hpp"
#include "launch.h"

namespace hlsp2p {
namespace dev {

// Passed by value as the first kernel parameter.  I32 / I64 as in es::IndexTables: const where the
// kernel only reads the index (EsBatchView); es_finish_kernel writes all four tables, sample_aes.hip
// nal.  remux_plan_kernel and the two of sample_aes.hip take the fields as separate `__restrict__`
// parameters instead and make the view themselves: their uniform loads stay scalar only so.
template <class I32, class I64>
struct EsBatchViewOf {
  const uint8_t* es;
  int64_t es_numel;
  const int64_t *es_off, *cap, *info, *pes;
  int64_t max_pes, max_nal;
  es::IndexTables<I32, I64> ix;
};
using EsBatchView = EsBatchViewOf<const int32_t, const int64_t>;

template <class I32 = const int32_t, class I64 = const int64_t>
inline EsBatchViewOf<I32, I64> es_batch_view(const EsBatch& b) {
  return {b.es, b.es_numel, b.es_off, b.cap, b.info, b.pes, b.max_pes, b.max_nal,
          {b.ix.nal, b.ix.au, b.ix.aframes, b.ix.sinfo}};
}

// Segment seg with the cap clamped to [0, 2^31): offsets inside a segment fit an int.  For a
// caller that wants no rows, or none yet.
template <class I32, class I64>
__device__ __forceinline__ es::Segment es_segment_clamped(const EsBatchViewOf<I32, I64>& b, int seg) {
  es::Segment sg = es::segment_at(b.es, b.es_off, b.cap, b.info, b.pes, b.max_pes, b.max_nal, seg);
  sg.cap = clamp(sg.cap, 0, 0x7fffffff);
  return sg;
}

// What a kernel takes from one segment of an indexed batch.
template <class I32, class I64>
struct EsSegmentView {
  es::Segment sg;                // es_segment_clamped
  es::IndexTables<I32, I64> ix;  // the segment's rows
  es::VideoSpan video;
  int64_t R, m;  // NAL rows and access units: the index's counts, clamped to max_nal / max_pes
  int cap;       // sg.cap
};
template <class I32, class I64>
__device__ __forceinline__ EsSegmentView<I32, I64> es_segment(const EsBatchViewOf<I32, I64>& b, int seg) {
  EsSegmentView<I32, I64> c;
  c.sg = es_segment_clamped(b, seg);
  c.ix = es::index_tables_at(b.ix, c.sg, seg);
  c.video = es::video_span(c.sg);
  c.R = es::video_rows(c.video, c.ix.sinfo[es::kNumNal], b.max_nal);
  c.m = es::video_rows(c.video, c.ix.sinfo[es::kNumAu], b.max_pes);
  c.cap = static_cast<int>(c.sg.cap);
  return c;
}

// Segment seg's ES as a buffer resource that ends with the ES tensor (at most 2^31 - 1 bytes on):
// a load through it can never leave the tensor, and reads zero beyond it.
template <class I32, class I64>
__device__ __forceinline__ __amdgpu_buffer_rsrc_t es_segment_rsrc(const EsBatchViewOf<I32, I64>& b, int seg) {
  const int64_t off = b.es_off[seg];
  const int64_t avail = b.es_numel - off;
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t*>(b.es + off), 0,
                                           static_cast<int>(avail < 0x7fffffff ? avail : 0x7fffffff), 0x00020000);
}

}  // namespace dev
}  // namespace hlsp2p
