// torch binding module `_C`: argument checking + current-HIP-stream launch of the gfx950
// kernels, as pybind functions and as dispatcher ops (torch.ops.hlsp2p.*).  Host-only
// translation unit; kernels live in *.hip objects.
#include <functional>
#include <initializer_list>
#include <type_traits>

#include "host_util.h"

namespace {

using torch::Tensor;
namespace D = hlsp2p::dev;
namespace ts = hlsp2p::ts;
namespace es_ = hlsp2p::es;  // `es` names a tensor below
namespace crc = hlsp2p::crc;
using hlsp2p::host::hip_ok;
using hlsp2p::host::num_cus;

// A launch field's pointer comes from its tensor's check; T fixes the dtype (uint32_t: int32 bits).
template <typename T>
T* check(const Tensor& t, const char* name, int64_t min_numel = 0) {
  constexpr c10::ScalarType dt = sizeof(T) == 8 ? torch::kInt64 : sizeof(T) == 4 ? torch::kInt32
                                 : std::is_signed<T>::value ? torch::kInt8 : torch::kUInt8;
  TORCH_CHECK(t.is_cuda(), name, " must be a GPU tensor");
  TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
  TORCH_CHECK(t.scalar_type() == dt, name, " has dtype ", t.scalar_type(), ", expected ", dt);
  TORCH_CHECK(t.numel() >= min_numel, name, " too small: ", t.numel(), " < ", min_numel);
  return static_cast<T*>(t.data_ptr());
}

hipStream_t stream() { return c10::hip::getCurrentHIPStream().stream(); }

// Device and alignment checks: es_batch below makes them of the batch's tensors, each op of its own.
void same_device(const Tensor& first, std::initializer_list<std::reference_wrapper<const Tensor>> rest) {
  for (const Tensor& t : rest) TORCH_CHECK(first.device() == t.device(), "tensors on different devices");
}
struct NamedTensor {
  const Tensor& t;
  const char* name;
};
void aligned16(std::initializer_list<NamedTensor> ts) {
  for (const NamedTensor& n : ts)
    TORCH_CHECK((reinterpret_cast<uintptr_t>(n.t.data_ptr()) & 15) == 0, n.name, " must be 16-byte aligned");
}

void aes128_cbc_decrypt(Tensor src, Tensor dst, Tensor src_off, Tensor dst_off, Tensor blk_prefix,
                        Tensor chunk_prefix, Tensor drk, Tensor iv, Tensor td0, Tensor isb, Tensor out_len,
                        int64_t total_chunks) {
  const int64_t B = src_off.numel();
  const D::AesDecryptArgs a{.src = check<uint8_t>(src, "src"),
                            .dst = check<uint8_t>(dst, "dst"),
                            .src_off = check<int64_t>(src_off, "src_off"),
                            .dst_off = check<int64_t>(dst_off, "dst_off", B),
                            .blk_prefix = check<int64_t>(blk_prefix, "blk_prefix", B + 1),
                            .chunk_prefix = check<int64_t>(chunk_prefix, "chunk_prefix", B + 1),
                            .drk = check<uint32_t>(drk, "drk", B * 44),
                            .iv = reinterpret_cast<const uint32_t*>(check<uint8_t>(iv, "iv", B * 16)),
                            .td0 = check<uint32_t>(td0, "td0", 256),
                            .isb = check<uint8_t>(isb, "isb", 256),
                            .out_len = check<int64_t>(out_len, "out_len", B),
                            .nseg = static_cast<int>(B), .total_chunks = total_chunks,
                            .num_cu = num_cus(src.get_device()), .stream = stream()};
  TORCH_CHECK(src.data_ptr() != dst.data_ptr(), "CBC decrypt cannot run in place");
  TORCH_CHECK((reinterpret_cast<uintptr_t>(src.data_ptr()) & 15) == 0 &&
                  (reinterpret_cast<uintptr_t>(dst.data_ptr()) & 15) == 0,
              "src/dst must be 16-byte aligned");
  TORCH_CHECK(src.device() == dst.device(), "tensors on different devices");
  hip_ok(D::launch_aes128_cbc_decrypt(a), "aes128_cbc_decrypt launch");
}

void crc32_batch(Tensor buf, Tensor seg_off, Tensor seg_len, Tensor tile_prefix, Tensor res_off, Tensor wfrag,
                 Tensor tables, Tensor residues, Tensor crc_out, c10::optional<Tensor> expect,
                 c10::optional<Tensor> ok_out, int64_t total_tiles, c10::optional<Tensor> scatter_idx,
                 c10::optional<Tensor> scatter_out) {
  const int64_t B = seg_off.numel();
  // B fragments pick the matrix-core path: int8 [64 steps][64 lanes][16] for the i8 MFMA,
  // uint8 [32][64][16] of packed e2m1 nibbles for the FP4 f8f6f4 MFMA
  const bool fp4 = wfrag.scalar_type() == torch::kUInt8;
  D::Crc32BatchArgs a{.buf = check<uint8_t>(buf, "buf"),
                      .seg_off = check<int64_t>(seg_off, "seg_off"),
                      .seg_len = check<int64_t>(seg_len, "seg_len", B),
                      .tile_prefix = check<int64_t>(tile_prefix, "tile_prefix", B + 1),
                      .res_off = check<int64_t>(res_off, "res_off", B),
                      .wfrag = fp4 ? static_cast<const void*>(check<uint8_t>(wfrag, "wfrag", 32 * 64 * 16))
                                    : check<int8_t>(wfrag, "wfrag", 64 * 64 * 16),
                      .fp4 = fp4,
                      .tables = check<uint32_t>(tables, "tables", crc::kShiftTableWords),
                      .residues = check<uint32_t>(residues, "residues"),
                      .out = {.crc_out = check<uint32_t>(crc_out, "crc_out", B)},
                      .nseg = static_cast<int>(B), .total_tiles = total_tiles, .num_cu = num_cus(buf.get_device()),
                      .stream = stream()};
  TORCH_CHECK((reinterpret_cast<uintptr_t>(buf.data_ptr()) & 15) == 0, "buf must be 16-byte aligned");
  if (expect.has_value()) a.out.expect = check<uint32_t>(*expect, "expect", B);
  if (ok_out.has_value()) a.out.ok_out = check<uint8_t>(*ok_out, "ok_out", B);
  TORCH_CHECK(scatter_idx.has_value() == scatter_out.has_value(), "scatter_idx and scatter_out go together");
  if (scatter_out.has_value()) {
    a.out.scatter_idx = check<int64_t>(*scatter_idx, "scatter_idx", B);
    a.out.scatter_out = check<uint32_t>(*scatter_out, "scatter_out");
    a.out.scatter_n = scatter_out->numel();
  }
  hip_ok(D::launch_crc32_batch(a), "crc32_batch launch");
}

void ts_demux(Tensor buf, Tensor seg_off, Tensor seg_len, Tensor blk_prefix, int64_t total_blocks, Tensor meta,
              Tensor pts_dts, Tensor blk_sums, Tensor es, Tensor es_off, Tensor pes, int64_t max_pes, Tensor info) {
  const int64_t B = seg_off.numel();
  const auto ws = ts::demux_workspace(total_blocks, B);
  const D::TsDemuxArgs a{.buf = check<uint8_t>(buf, "buf"),
                         .seg_off = check<int64_t>(seg_off, "seg_off"),
                         .seg_len = check<int64_t>(seg_len, "seg_len", B),
                         .blk_prefix = check<int64_t>(blk_prefix, "blk_prefix", B + 1),
                         .nseg = static_cast<int>(B), .total_blocks = total_blocks,
                         .meta = check<uint32_t>(meta, "meta", ws.meta),
                         .pts_dts = check<int64_t>(pts_dts, "pts_dts", ws.pts_dts),
                         .aux = check<int32_t>(blk_sums, "aux", ws.aux),
                         .es = check<uint8_t>(es, "es"),
                         .es_off = check<int64_t>(es_off, "es_off", B),
                         .pes = check<int64_t>(pes, "pes", ts::pes_words(B, max_pes)),
                         .max_pes = max_pes,
                         .info = check<int64_t>(info, "info", B * ts::kInfoWords),
                         .stream = stream()};
  TORCH_CHECK((reinterpret_cast<uintptr_t>(buf.data_ptr()) & 15) == 0, "buf must be 16-byte aligned");
  hip_ok(D::launch_ts_demux(a), "ts_demux launch");
}

// The demuxed (and, behind es_index, indexed) batch every op below takes (launch.h EsBatch), checked
// here for all of them: max_pes / max_nal / total_tiles in range (`op` names the caller), every
// tensor a contiguous GPU tensor of its dtype and size, all of them on one device, es and nal
// 16-byte aligned.  es / info / pes are ts_demux's outputs, cap the host upper bound of each
// segment's ES bytes (the Python wrapper has checked es_off + cap against es), tile_prefix the
// exclusive prefix of the op's tiles per segment.  An op without a tile space (codec_config)
// passes no tile_prefix and 0 tiles.  What is left to an op: its own tensors and sizes.
D::EsBatch es_batch(const char* op, const Tensor& es, const Tensor& es_off, const Tensor& cap,
                    const c10::optional<Tensor>& tile_prefix, int64_t total_tiles, const Tensor& info, const Tensor& pes,
                    int64_t max_pes, int64_t max_nal, const Tensor& nal, const Tensor& au, const Tensor& aframes,
                    const Tensor& sinfo) {
  TORCH_CHECK(max_pes > 0 && max_pes <= 0x7fffffff && max_nal > 0 && max_nal <= 0x7fffffff && total_tiles >= 0, op,
              ": max_pes / max_nal / total_tiles out of range");
  const int64_t B = es_off.numel();
  const D::EsBatch b{
      .es = check<uint8_t>(es, "es"), .es_numel = es.numel(),
      .es_off = check<int64_t>(es_off, "es_off"),
      .cap = check<int64_t>(cap, "cap", B),
      .tile_prefix = tile_prefix.has_value() ? check<int64_t>(*tile_prefix, "tile_prefix", B + 1) : nullptr,
      .nseg = static_cast<int>(B), .total_tiles = total_tiles,
      .info = check<int64_t>(info, "info", B * ts::kInfoWords),
      .pes = check<int64_t>(pes, "pes", ts::pes_words(B, max_pes)),
      .max_pes = max_pes, .max_nal = max_nal,
      .ix = {check<int32_t>(nal, "nal", hlsp2p::table_words(B, max_nal, es_::kNalWords)),
             check<int32_t>(au, "au", hlsp2p::table_words(B, max_pes, es_::kAuWords)),
             check<int32_t>(aframes, "aframes", hlsp2p::table_words(B, max_pes, es_::kApesWords)),
             check<int64_t>(sinfo, "sinfo", B * es_::kSinfoWords)},
      .stream = stream()};
  same_device(es, {es_off, cap, info, pes, nal, au, aframes, sinfo});
  if (tile_prefix.has_value()) same_device(es, {*tile_prefix});
  aligned16({{es, "es"}, {nal, "nal"}});
  return b;
}

// Sample index of a demuxed batch (es_index.hip): tile_prefix counts ceil(cap / es_index_tile_bytes()).
void es_index(Tensor es, Tensor es_off, Tensor cap, Tensor tile_prefix, int64_t total_tiles, Tensor info, Tensor pes,
              int64_t max_pes, int64_t max_nal, Tensor scratch, Tensor nal, Tensor au, Tensor aframes, Tensor sinfo) {
  const D::EsIndexArgs a{
      .b = es_batch("es_index", es, es_off, cap, tile_prefix, total_tiles, info, pes, max_pes, max_nal, nal, au, aframes,
                    sinfo),
      .scratch = check<int32_t>(scratch, "scratch", es_::index_scratch(total_tiles, es_off.numel(), max_nal).end)};
  same_device(es, {scratch});
  hip_ok(D::launch_es_index(a), "es_index launch");
}

// Remux of a demuxed and indexed batch (remux.hip): the inputs of es_index, its four outputs, and
// per segment a region of es::remux_out_bytes(cap, max_nal) + audio_gap bytes of `out` at out_off (the
// Python wrapper has checked the regions against out); tile_prefix counts ceil(region / remux_tile_bytes()).
void remux(Tensor es, Tensor es_off, Tensor cap, Tensor tile_prefix, int64_t total_tiles, Tensor info, Tensor pes,
           int64_t max_pes, int64_t max_nal, Tensor nal, Tensor au, Tensor aframes, Tensor sinfo, int64_t max_aframes,
           Tensor scratch, Tensor vsamples, Tensor asamples, Tensor rinfo, Tensor out, Tensor out_off,
           int64_t audio_gap) {
  const int64_t B = es_off.numel();
  TORCH_CHECK(max_aframes > 0, "remux: max_aframes out of range");
  TORCH_CHECK(audio_gap >= 0 && audio_gap % 16 == 0 && audio_gap < (int64_t(1) << 30),
              "remux: audio_gap must be a non-negative multiple of 16");
  const D::RemuxArgs a{
      .b = es_batch("remux", es, es_off, cap, tile_prefix, total_tiles, info, pes, max_pes, max_nal, nal, au, aframes,
                    sinfo),
      .max_aframes = max_aframes,
      .scratch = check<int32_t>(scratch, "scratch", es_::remux_scratch(B, max_nal, max_aframes).end),
      .t = {check<int32_t>(vsamples, "vsamples", hlsp2p::table_words(B, max_pes, es_::kVsampleWords)),
            check<int32_t>(asamples, "asamples", hlsp2p::table_words(B, max_aframes, es_::kAsampleWords)),
            check<int64_t>(rinfo, "rinfo", B * es_::kRinfoWords)},
      .out = check<uint8_t>(out, "out"),
      .out_off = check<int64_t>(out_off, "out_off", B),
      .audio_gap = audio_gap};
  same_device(es, {scratch, vsamples, asamples, rinfo, out, out_off});
  aligned16({{out, "out"}});
  TORCH_CHECK(es.data_ptr() != out.data_ptr(), "remux cannot run in place");
  hip_ok(D::launch_remux(a), "remux launch");
}

// The moof boxes of a remuxed batch (fragment.hip): remux's three tables, es_index's sinfo, one
// fparams row per segment (the Python wrapper has checked the regions against out and against each
// other; the kernel leaves a row alone that does not lie inside out) and `out` as remux left it.
void fragment_moof(Tensor rinfo, Tensor vsamples, Tensor asamples, Tensor sinfo, Tensor fparams, int64_t max_pes,
                   int64_t max_aframes, int64_t headroom, int64_t audio_gap, Tensor out, Tensor finfo,
                   c10::optional<Tensor> mpainfo) {
  const int64_t B = fparams.numel() / es_::kFparamWords;
  TORCH_CHECK(max_pes > 0 && max_aframes > 0 && max_pes <= 0x7fffffff / 16 && max_aframes <= 0x7fffffff / 16,
              "fragment_moof: max_pes / max_aframes out of range");
  TORCH_CHECK(headroom >= es_::frag_headroom(max_pes), "fragment_moof: headroom below frag_headroom(max_pes)");
  TORCH_CHECK(audio_gap >= es_::frag_audio_gap(max_aframes) && audio_gap % 16 == 0,
              "fragment_moof: audio_gap below frag_audio_gap(max_aframes) or no multiple of 16");
  TORCH_CHECK(fparams.numel() == B * es_::kFparamWords, "fragment_moof: fparams is not a whole number of rows");
  const D::FragmentArgs a{
      .rinfo = check<int64_t>(rinfo, "rinfo", B * es_::kRinfoWords),
      .vsamples = check<int32_t>(vsamples, "vsamples", hlsp2p::table_words(B, max_pes, es_::kVsampleWords)),
      .asamples = check<int32_t>(asamples, "asamples", hlsp2p::table_words(B, max_aframes, es_::kAsampleWords)),
      .sinfo = check<int64_t>(sinfo, "sinfo", B * es_::kSinfoWords),
      .fparams = check<int64_t>(fparams, "fparams"),
      .max_pes = max_pes, .max_aframes = max_aframes, .headroom = headroom, .audio_gap = audio_gap,
      .out = check<uint8_t>(out, "out"), .out_numel = out.numel(),
      .finfo = check<int64_t>(finfo, "finfo", B * es_::kFinfoWords),
      .mpainfo = mpainfo.has_value() ? check<int64_t>(*mpainfo, "mpainfo", B * es_::kMpainfoWords) : nullptr,
      .nseg = static_cast<int>(B), .stream = stream()};
  same_device(out, {rinfo, vsamples, asamples, sinfo, fparams, finfo});
  if (mpainfo.has_value()) same_device(out, {*mpainfo});
  aligned16({{out, "out"}});
  hip_ok(D::launch_fragment_moof(a), "fragment_moof launch");
}

// MPEG audio of a demuxed and remuxed batch (mpeg_audio.hip): ts_demux's outputs, per segment the
// bytes of its output region (what remux was sized with; the Python wrapper has checked the regions
// against out), remux's asamples, rinfo and out, which are rewritten for a segment with an MPEG
// audio config; tile_prefix counts ceil(region / mpeg_audio_tile_bytes()).
void mpeg_audio(Tensor es, Tensor es_off, Tensor cap, Tensor tile_prefix, int64_t total_tiles, Tensor info, Tensor pes,
                int64_t max_pes, Tensor region, int64_t max_aframes, Tensor scratch, Tensor mframes, Tensor mpainfo,
                Tensor asamples, Tensor rinfo, Tensor out, Tensor out_off) {
  const int64_t B = es_off.numel();
  TORCH_CHECK(max_pes > 0 && max_pes <= 0x7fffffff / 4 && max_aframes > 0 && total_tiles >= 0,
              "mpeg_audio: max_pes / max_aframes / total_tiles out of range");
  const D::MpegAudioArgs a{
      .b = {.es = check<uint8_t>(es, "es"), .es_numel = es.numel(),
            .es_off = check<int64_t>(es_off, "es_off"),
            .cap = check<int64_t>(cap, "cap", B),
            .tile_prefix = check<int64_t>(tile_prefix, "tile_prefix", B + 1),
            .nseg = static_cast<int>(B), .total_tiles = total_tiles,
            .info = check<int64_t>(info, "info", B * ts::kInfoWords),
            .pes = check<int64_t>(pes, "pes", ts::pes_words(B, max_pes)),
            .max_pes = max_pes, .max_nal = 0, .ix = {nullptr, nullptr, nullptr, nullptr}, .stream = stream()},
      .region = check<int64_t>(region, "region", B),
      .max_aframes = max_aframes,
      .scratch = check<int32_t>(scratch, "scratch", es_::mpa_scratch(B, max_pes).end),
      .t = {check<int32_t>(mframes, "mframes", hlsp2p::table_words(B, max_pes, es_::kApesWords)),
            check<int64_t>(mpainfo, "mpainfo", B * es_::kMpainfoWords),
            check<int32_t>(asamples, "asamples", hlsp2p::table_words(B, max_aframes, es_::kAsampleWords)),
            check<int64_t>(rinfo, "rinfo", B * es_::kRinfoWords)},
      .out = check<uint8_t>(out, "out"),
      .out_off = check<int64_t>(out_off, "out_off", B)};
  same_device(es, {es_off, cap, tile_prefix, info, pes, region, scratch, mframes, mpainfo, asamples, rinfo, out, out_off});
  aligned16({{es, "es"}, {out, "out"}});
  TORCH_CHECK(es.data_ptr() != out.data_ptr(), "mpeg_audio cannot run in place");
  hip_ok(D::launch_mpeg_audio(a), "mpeg_audio launch");
}

// AC-3 / E-AC-3 audio of a demuxed and remuxed batch (ac3_audio.hip): mpeg_audio's arguments, with
// ac3info and a new tensor in mpainfo's layout; mpa_in is mpeg_audio's mpainfo (only read) or None.
void ac3_audio(Tensor es, Tensor es_off, Tensor cap, Tensor tile_prefix, int64_t total_tiles, Tensor info, Tensor pes,
               int64_t max_pes, Tensor region, int64_t max_aframes, Tensor scratch, Tensor dframes, Tensor ac3info,
               Tensor mpainfo, Tensor asamples, Tensor rinfo, Tensor out, Tensor out_off,
               const c10::optional<Tensor>& mpa_in) {
  const int64_t B = es_off.numel();
  TORCH_CHECK(max_pes > 0 && max_pes <= 0x7fffffff / 4 && max_aframes > 0 && total_tiles >= 0,
              "ac3_audio: max_pes / max_aframes / total_tiles out of range");
  const D::Ac3AudioArgs a{
      .b = {.es = check<uint8_t>(es, "es"), .es_numel = es.numel(),
            .es_off = check<int64_t>(es_off, "es_off"),
            .cap = check<int64_t>(cap, "cap", B),
            .tile_prefix = check<int64_t>(tile_prefix, "tile_prefix", B + 1),
            .nseg = static_cast<int>(B), .total_tiles = total_tiles,
            .info = check<int64_t>(info, "info", B * ts::kInfoWords),
            .pes = check<int64_t>(pes, "pes", ts::pes_words(B, max_pes)),
            .max_pes = max_pes, .max_nal = 0, .ix = {nullptr, nullptr, nullptr, nullptr}, .stream = stream()},
      .region = check<int64_t>(region, "region", B),
      .max_aframes = max_aframes,
      .scratch = check<int32_t>(scratch, "scratch", es_::mpa_scratch(B, max_pes).end),
      .t = {check<int32_t>(dframes, "dframes", hlsp2p::table_words(B, max_pes, es_::kApesWords)),
            check<int64_t>(ac3info, "ac3info", B * es_::kAc3infoWords),
            check<int64_t>(mpainfo, "mpainfo", B * es_::kMpainfoWords),
            mpa_in.has_value() ? check<int64_t>(*mpa_in, "mpa_in", B * es_::kMpainfoWords) : nullptr,
            check<int32_t>(asamples, "asamples", hlsp2p::table_words(B, max_aframes, es_::kAsampleWords)),
            check<int64_t>(rinfo, "rinfo", B * es_::kRinfoWords)},
      .out = check<uint8_t>(out, "out"),
      .out_off = check<int64_t>(out_off, "out_off", B)};
  same_device(es, {es_off, cap, tile_prefix, info, pes, region, scratch, dframes, ac3info, mpainfo, asamples, rinfo, out,
                   out_off});
  if (mpa_in.has_value()) {
    same_device(es, {*mpa_in});
    TORCH_CHECK(mpa_in->data_ptr() != mpainfo.data_ptr(), "ac3_audio: mpainfo must not be mpa_in");
  }
  aligned16({{es, "es"}, {out, "out"}});
  TORCH_CHECK(es.data_ptr() != out.data_ptr(), "ac3_audio cannot run in place");
  hip_ok(D::launch_ac3_audio(a), "ac3_audio launch");
}

// Codec configuration of a demuxed and indexed batch (codec_config.hip): the inputs of es_index
// without a tile space, its four outputs, and per segment a cinfo row and two rows of max_ps bytes.
void codec_config(Tensor es, Tensor es_off, Tensor cap, Tensor info, Tensor pes, int64_t max_pes, int64_t max_nal,
                  Tensor nal, Tensor au, Tensor aframes, Tensor sinfo, int64_t max_ps, Tensor cinfo, Tensor ps) {
  const int64_t B = es_off.numel();
  TORCH_CHECK(es_::max_ps_ok(max_ps), "codec_config: max_ps must be a positive multiple of 16 up to 1024");
  const D::CodecConfigArgs a{
      .b = es_batch("codec_config", es, es_off, cap, c10::nullopt, 0, info, pes, max_pes, max_nal, nal, au, aframes,
                    sinfo),
      .max_ps = max_ps,
      .ps = check<uint8_t>(ps, "ps", es_::ps_bytes(B, max_ps)),
      .cinfo = check<int32_t>(cinfo, "cinfo", B * es_::kCinfoWords)};
  same_device(es, {ps, cinfo});
  aligned16({{ps, "ps"}});
  hip_ok(D::launch_codec_config(a), "codec_config launch");
}

// HEVC configuration of a demuxed and indexed batch (hevc_config.hip): the inputs of codec_config,
// and per segment an hinfo row and three rows of max_ps bytes.
void hevc_config(Tensor es, Tensor es_off, Tensor cap, Tensor info, Tensor pes, int64_t max_pes, int64_t max_nal,
                 Tensor nal, Tensor au, Tensor aframes, Tensor sinfo, int64_t max_ps, Tensor hinfo, Tensor hps) {
  const int64_t B = es_off.numel();
  TORCH_CHECK(es_::max_ps_ok(max_ps), "hevc_config: max_ps must be a positive multiple of 16 up to 1024");
  const D::HevcConfigArgs a{
      .b = es_batch("hevc_config", es, es_off, cap, c10::nullopt, 0, info, pes, max_pes, max_nal, nal, au, aframes,
                    sinfo),
      .max_ps = max_ps,
      .hps = check<uint8_t>(hps, "hps", es_::hps_bytes(B, max_ps)),
      .hinfo = check<int32_t>(hinfo, "hinfo", B * es_::kHinfoWords)};
  same_device(es, {hps, hinfo});
  aligned16({{hps, "hps"}});
  hip_ok(D::launch_hevc_config(a), "hevc_config launch");
}

// SAMPLE-AES decryption of a demuxed and indexed batch in place (sample_aes.hip): the inputs of
// codec_config, of which es and the length column of nal are rewritten; per segment 44 round-key
// words (little-endian), a 16-byte IV and an enable byte; td / isb are ops.aes.device_tables.
void sample_aes_decrypt(Tensor es, Tensor es_off, Tensor cap, Tensor info, Tensor pes, int64_t max_pes, int64_t max_nal,
                        Tensor nal, Tensor au, Tensor aframes, Tensor sinfo, Tensor round_keys, Tensor iv, Tensor enable,
                        Tensor td, Tensor isb, Tensor sainfo) {
  const int64_t B = es_off.numel();
  TORCH_CHECK(B <= 65535, "sample_aes_decrypt: at most 65535 segments per call");
  const D::SampleAesArgs a{
      .b = es_batch("sample_aes_decrypt", es, es_off, cap, c10::nullopt, 0, info, pes, max_pes, max_nal, nal, au,
                    aframes, sinfo),
      .es = check<uint8_t>(es, "es"),
      .round_keys = check<uint32_t>(round_keys, "round_keys", B * es_::kAesRoundKeyWords),
      .iv = check<uint8_t>(iv, "iv", B * es_::kAesBlock),
      .enable = check<uint8_t>(enable, "enable", B),
      .td = check<uint32_t>(td, "td", 256),
      .isb = check<uint8_t>(isb, "isb", 256),
      .sainfo = check<int64_t>(sainfo, "sainfo", B * es_::kSaWords)};
  same_device(es, {round_keys, iv, enable, td, isb, sainfo});
  aligned16({{iv, "iv"}});
  hip_ok(D::launch_sample_aes(a), "sample_aes_decrypt launch");
}

// Caption extraction of a demuxed and indexed batch (captions.hip): the inputs of codec_config, all
// only read, an enable byte per segment, es::cc_scratch(B, max_nal) words of scratch, and the five
// caption tables of max_cc rows per segment.
void cc_extract(Tensor es, Tensor es_off, Tensor cap, Tensor info, Tensor pes, int64_t max_pes, int64_t max_nal,
                Tensor nal, Tensor au, Tensor aframes, Tensor sinfo, Tensor enable, int64_t max_cc, Tensor scratch,
                Tensor ccsamples, Tensor ccpts, Tensor ccbytes, Tensor cc608, Tensor ccinfo) {
  const int64_t B = es_off.numel();
  TORCH_CHECK(es_::max_cc_ok(max_cc), "cc_extract: max_cc must be 1 to 2048");
  TORCH_CHECK(B <= 65535, "cc_extract: at most 65535 segments per call");
  const D::CcExtractArgs a{
      .b = es_batch("cc_extract", es, es_off, cap, c10::nullopt, 0, info, pes, max_pes, max_nal, nal, au, aframes, sinfo),
      .enable = check<uint8_t>(enable, "enable", B),
      .max_cc = max_cc,
      .scratch = check<int32_t>(scratch, "scratch", es_::cc_scratch(B, max_nal).end),
      .t = {check<int32_t>(ccsamples, "ccsamples", hlsp2p::table_words(B, max_cc, es_::kCcRowWords)),
            check<int64_t>(ccpts, "ccpts", B * max_cc),
            check<uint8_t>(ccbytes, "ccbytes", B * max_cc * es_::kCcSlotBytes),
            check<uint8_t>(cc608, "cc608", B * max_cc * 2 * es_::kCcFieldBytes),
            check<int64_t>(ccinfo, "ccinfo", B * es_::kCcInfoWords)}};
  same_device(es, {enable, scratch, ccsamples, ccpts, ccbytes, cc608, ccinfo});
  aligned16({{scratch, "scratch"}, {ccsamples, "ccsamples"}, {ccbytes, "ccbytes"}, {cc608, "cc608"}});
  hip_ok(D::launch_cc_extract(a), "cc_extract launch");
}

// Demux of fragmented-MP4 segments (mp4_demux.hip): segment i is buf[off[i], off[i] + clamp(len[i], 0,
// cap[i])) (the Python wrapper has checked off + cap against buf), tracks int64[B, 2, 8]; ten output
// tables, info / pes in ts_demux's layout and nal / au / aframes / sinfo in es_index's.
void mp4_demux(Tensor buf, Tensor off, Tensor len, Tensor cap, Tensor tracks, int64_t max_pes, int64_t max_nal,
               int64_t max_moof, int64_t max_run, int64_t max_emsg, Tensor minfo, Tensor msamples, Tensor runs,
               Tensor emsg, Tensor info, Tensor pes, Tensor nal, Tensor au, Tensor aframes, Tensor sinfo) {
  namespace mp4 = hlsp2p::mp4;
  const int64_t B = off.numel();
  TORCH_CHECK(max_pes > 0 && max_pes <= 0x7fffffff && max_nal > 0 && max_nal <= 0x7fffffff,
              "mp4_demux: max_pes / max_nal out of range");
  TORCH_CHECK(mp4::max_rows_ok(max_moof) && mp4::max_rows_ok(max_run) && mp4::max_rows_ok(max_emsg),
              "mp4_demux: max_moof / max_run / max_emsg must be 1 to 256");
  const D::Mp4DemuxArgs a{
      .buf = check<uint8_t>(buf, "buf"), .buf_numel = buf.numel(),
      .off = check<int64_t>(off, "off"),
      .len = check<int64_t>(len, "len", B),
      .cap = check<int64_t>(cap, "cap", B),
      .tracks = check<int64_t>(tracks, "tracks", B * mp4::kTracks * mp4::kTrackWords),
      .nseg = static_cast<int>(B),
      .lim = {max_pes, max_nal, max_moof, max_run, max_emsg},
      .t = {check<int64_t>(minfo, "minfo", B * mp4::kMinfoWords),
            check<int32_t>(msamples, "msamples", hlsp2p::table_words(B, mp4::kTracks * max_pes, mp4::kMsampleWords)),
            check<int64_t>(runs, "runs", hlsp2p::table_words(B, max_run, mp4::kRunWords)),
            check<int64_t>(emsg, "emsg", hlsp2p::table_words(B, max_emsg, mp4::kEmsgWords)),
            check<int64_t>(info, "info", B * ts::kInfoWords),
            check<int64_t>(pes, "pes", ts::pes_words(B, max_pes)),
            {check<int32_t>(nal, "nal", hlsp2p::table_words(B, max_nal, es_::kNalWords)),
             check<int32_t>(au, "au", hlsp2p::table_words(B, max_pes, es_::kAuWords)),
             check<int32_t>(aframes, "aframes", hlsp2p::table_words(B, max_pes, es_::kApesWords)),
             check<int64_t>(sinfo, "sinfo", B * es_::kSinfoWords)}},
      .stream = stream()};
  same_device(buf, {off, len, cap, tracks, minfo, msamples, runs, emsg, info, pes, nal, au, aframes, sinfo});
  aligned16({{buf, "buf"}, {msamples, "msamples"}, {runs, "runs"}, {emsg, "emsg"}, {nal, "nal"}, {au, "au"},
             {aframes, "aframes"}});
  hip_ok(D::launch_mp4_demux(a), "mp4_demux launch");
}

// Demux of packed-audio segments (packed_audio.hip): segment i is buf[off[i], off[i] + clamp(len[i], 0,
// cap[i])) (the Python wrapper has checked off + cap against buf); seven output tables, info / pes in
// ts_demux's layout and nal (one row) / au / aframes / sinfo in es_index's.  staged = false walks the
// frame chain in global memory: the variant tools/kernel_bench.py measures the LDS walk against.
void packed_audio(Tensor buf, Tensor off, Tensor len, Tensor cap, int64_t max_pes, Tensor info, Tensor pes, Tensor nal,
                  Tensor au, Tensor aframes, Tensor sinfo, Tensor painfo, bool staged) {
  const int64_t B = off.numel();
  TORCH_CHECK(es_::packed_max_pes_ok(max_pes), "packed_audio: max_pes must be 1 to ", es_::kPackedMaxPesLimit);
  const D::PackedAudioArgs a{
      .buf = check<uint8_t>(buf, "buf"), .buf_numel = buf.numel(),
      .off = check<int64_t>(off, "off"),
      .len = check<int64_t>(len, "len", B),
      .cap = check<int64_t>(cap, "cap", B),
      .nseg = static_cast<int>(B),
      .max_pes = max_pes,
      .t = {check<int64_t>(info, "info", B * ts::kInfoWords),
            check<int64_t>(pes, "pes", ts::pes_words(B, max_pes)),
            {check<int32_t>(nal, "nal", hlsp2p::table_words(B, es_::kPackedNalRows, es_::kNalWords)),
             check<int32_t>(au, "au", hlsp2p::table_words(B, max_pes, es_::kAuWords)),
             check<int32_t>(aframes, "aframes", hlsp2p::table_words(B, max_pes, es_::kApesWords)),
             check<int64_t>(sinfo, "sinfo", B * es_::kSinfoWords)},
            check<int64_t>(painfo, "painfo", B * es_::kPainfoWords)},
      .staged = staged,
      .stream = stream()};
  same_device(buf, {off, len, cap, info, pes, nal, au, aframes, sinfo, painfo});
  aligned16({{buf, "buf"}, {nal, "nal"}, {au, "au"}, {aframes, "aframes"}});
  hip_ok(D::launch_packed_audio(a), "packed_audio launch");
}

// cbcs decryption of a demuxed fMP4 batch into a copy (cbcs.hip): src and the five demux tables are
// only read; dst already holds a copy of every enabled segment at dst_off[i] (the Python wrapper
// has checked both offset sets against their tensors); per segment two protection rows, two
// constant IVs, a fallback IV, 44 round-key words (little-endian) and an enable byte.
// (shared with cenc_decrypt below: range_words and info_words are the scheme's row widths)
D::CbcsArgs protected_args(const char* op, int range_words, int info_words, Tensor src, Tensor src_off, Tensor cap,
                           Tensor dst, Tensor dst_off, Tensor info, Tensor pes, Tensor minfo, Tensor msamples,
                           Tensor runs, int64_t max_pes, int64_t max_run, Tensor prot, Tensor const_iv, Tensor iv,
                           Tensor round_keys, Tensor enable, Tensor td, Tensor isb, int64_t max_range,
                           int64_t max_blocks, Tensor scratch, Tensor ranges, Tensor cinfo) {
  namespace mp4 = hlsp2p::mp4;
  const int64_t B = src_off.numel();
  TORCH_CHECK(B <= 65535, op, ": at most 65535 segments per call");
  TORCH_CHECK(max_pes > 0 && max_pes < (int64_t(1) << mp4::kRgTrackShift) && mp4::max_rows_ok(max_run),
              op, ": max_pes / max_run out of range");
  TORCH_CHECK(mp4::max_range_ok(max_range), op, ": max_range must be 1 to 65536");
  TORCH_CHECK(max_blocks >= 0 && max_blocks <= 0x7fffffff / 16, op, ": max_blocks out of range");
  const D::CbcsArgs a{
      .src = check<uint8_t>(src, "src"), .src_numel = src.numel(),
      .src_off = check<int64_t>(src_off, "src_off"),
      .cap = check<int64_t>(cap, "cap", B),
      .dst = check<uint8_t>(dst, "dst"),
      .dst_off = check<int64_t>(dst_off, "dst_off", B),
      .info = check<int64_t>(info, "info", B * ts::kInfoWords),
      .pes = check<int64_t>(pes, "pes", ts::pes_words(B, max_pes)),
      .minfo = check<int64_t>(minfo, "minfo", B * mp4::kMinfoWords),
      .runs = check<int64_t>(runs, "runs", hlsp2p::table_words(B, max_run, mp4::kRunWords)),
      .msamples = check<int32_t>(msamples, "msamples", hlsp2p::table_words(B, mp4::kTracks * max_pes, mp4::kMsampleWords)),
      .max_pes = max_pes, .max_run = max_run,
      .prot = check<int64_t>(prot, "prot", B * mp4::kTracks * mp4::kProtWords),
      .const_iv = check<uint8_t>(const_iv, "const_iv", B * mp4::kTracks * es_::kAesBlock),
      .iv = check<uint8_t>(iv, "iv", B * es_::kAesBlock),
      .round_keys = check<uint32_t>(round_keys, "round_keys", B * es_::kAesRoundKeyWords),
      .enable = check<uint8_t>(enable, "enable", B),
      .td = check<uint32_t>(td, "td", 256),
      .isb = check<uint8_t>(isb, "isb", 256),
      .max_range = max_range, .max_blocks = max_blocks,
      .scratch = check<int32_t>(scratch, "scratch", mp4::cbcs_scratch(B, max_pes)),
      .ranges = check<int32_t>(ranges, "ranges", hlsp2p::table_words(B, max_range, range_words)),
      .cinfo = check<int64_t>(cinfo, "cinfo", B * info_words),
      .nseg = static_cast<int>(B), .stream = stream()};
  TORCH_CHECK(src.data_ptr() != dst.data_ptr(), op, " cannot run in place");
  same_device(src, {src_off, cap, dst, dst_off, info, pes, minfo, msamples, runs, prot, const_iv, iv, round_keys, enable,
                    td, isb, scratch, ranges, cinfo});
  aligned16({{src, "src"}, {dst, "dst"}, {msamples, "msamples"}, {const_iv, "const_iv"}, {iv, "iv"},
             {scratch, "scratch"}, {ranges, "ranges"}, {cinfo, "cinfo"}});
  return a;
}
void cbcs_decrypt(Tensor src, Tensor src_off, Tensor cap, Tensor dst, Tensor dst_off, Tensor info, Tensor pes,
                  Tensor minfo, Tensor msamples, Tensor runs, int64_t max_pes, int64_t max_run, Tensor prot,
                  Tensor const_iv, Tensor iv, Tensor round_keys, Tensor enable, Tensor td, Tensor isb, int64_t max_range,
                  int64_t max_blocks, Tensor scratch, Tensor ranges, Tensor cinfo) {
  namespace mp4 = hlsp2p::mp4;
  hip_ok(D::launch_cbcs(protected_args("cbcs_decrypt", mp4::kRangeWords, mp4::kCbInfoWords, src, src_off, cap, dst,
                                       dst_off, info, pes, minfo, msamples, runs, max_pes, max_run, prot, const_iv, iv,
                                       round_keys, enable, td, isb, max_range, max_blocks, scratch, ranges, cinfo)),
         "cbcs_decrypt launch");
}

// cenc (AES-CTR) decryption of a demuxed fMP4 batch into a copy (cenc.hip): the arguments of
// cbcs_decrypt with the 44 forward round-key words (little-endian), te the forward table TeL, sbox
// the S-box, and max_cap the largest cap of an enabled segment.
void cenc_decrypt(Tensor src, Tensor src_off, Tensor cap, Tensor dst, Tensor dst_off, Tensor info, Tensor pes,
                  Tensor minfo, Tensor msamples, Tensor runs, int64_t max_pes, int64_t max_run, Tensor prot,
                  Tensor const_iv, Tensor iv, Tensor round_keys, Tensor enable, Tensor te, Tensor sbox, int64_t max_range,
                  int64_t max_cap, Tensor scratch, Tensor ranges, Tensor cinfo) {
  namespace mp4 = hlsp2p::mp4;
  TORCH_CHECK(max_cap >= 0 && max_cap < 0x7fffffff - 64, "cenc_decrypt: max_cap out of range");
  const D::CencArgs a{protected_args("cenc_decrypt", mp4::kCnRangeWords, mp4::kCnInfoWords, src, src_off, cap, dst,
                                     dst_off, info, pes, minfo, msamples, runs, max_pes, max_run, prot, const_iv, iv,
                                     round_keys, enable, te, sbox, max_range, 0, scratch, ranges, cinfo),
                      max_cap, num_cus(src.get_device())};
  hip_ok(D::launch_cenc(a), "cenc_decrypt launch");
}

void segment_copy(Tensor src, Tensor dst, Tensor src_off, Tensor dst_off, Tensor len, Tensor chunk_prefix,
                  int64_t total_chunks) {
  const int64_t n = src_off.numel();
  hip_ok(D::launch_segment_copy({.src = check<uint8_t>(src, "src"),
                                 .dst = check<uint8_t>(dst, "dst"),
                                 .src_off = check<int64_t>(src_off, "src_off"),
                                 .dst_off = check<int64_t>(dst_off, "dst_off", n),
                                 .len = check<int64_t>(len, "len", n),
                                 .chunk_prefix = check<int64_t>(chunk_prefix, "chunk_prefix", n + 1),
                                 .ncopy = static_cast<int>(n), .total_chunks = total_chunks, .stream = stream()}),
         "segment_copy launch");
}

int64_t device_cus(Tensor t) { return num_cus(t.get_device()); }

// CDN ingest: pinned host -> HBM arena on the current stream, issued in one native call.
// Copies whose source (same pinned allocation, src_alloc[i]) and destination advance by the
// same delta, with a gap below max_gap, are merged into one DMA: a round's segments sit
// back to back in both the origin pool and the arena run (same 256-B alignment), and one
// 192 MB copy moves at ~57 GB/s where 64 x 3 MB copies reach ~48 GB/s on MI355X.
// A gap below the arena alignment is the previous entry's own padding (entries start on
// aligned offsets), so a merged copy never touches another entry.  Returns #DMAs issued.
// device_src: the sources are HBM (a diagnostic origin kept on the GPU, standing in for
// segments that arrive over xGMI), so the copies are device-to-device.
int64_t h2d_batch(Tensor dst, pybind11::array_t<int64_t> dst_off, pybind11::array_t<int64_t> src_ptr,
                  pybind11::array_t<int64_t> len, pybind11::array_t<int64_t> src_alloc, int64_t max_gap,
                  bool device_src) {
  uint8_t* base = check<uint8_t>(dst, "dst");
  const int64_t n = dst_off.size();
  TORCH_CHECK(src_ptr.size() == n && len.size() == n && src_alloc.size() == n, "h2d_batch: argument sizes differ");
  const int64_t* o = dst_off.data();
  const int64_t* s = src_ptr.data();
  const int64_t* l = len.data();
  const int64_t* a = src_alloc.data();
  const int64_t cap = dst.numel();
  hipStream_t st = stream();
  int64_t issued = 0;
  int64_t i = 0;
  while (i < n) {
    TORCH_CHECK(o[i] >= 0 && l[i] >= 0 && o[i] + l[i] <= cap, "h2d_batch: destination out of bounds");
    if (l[i] == 0) {
      ++i;
      continue;
    }
    int64_t j = i;
    while (j + 1 < n && l[j + 1] > 0 && a[j + 1] == a[j]) {
      const int64_t ds = o[j + 1] - o[j], ss = s[j + 1] - s[j];
      if (ds != ss || ds < l[j] || ds - l[j] >= max_gap) break;
      TORCH_CHECK(o[j + 1] + l[j + 1] <= cap, "h2d_batch: destination out of bounds");
      ++j;
    }
    const int64_t bytes = o[j] + l[j] - o[i];
    hip_ok(hipMemcpyAsync(base + o[i], reinterpret_cast<const void*>(s[i]), static_cast<size_t>(bytes),
                          device_src ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st),
           "hipMemcpyAsync launch");
    ++issued;
    i = j + 1;
  }
  return issued;
}

// Kernel-argument descriptors (ops/desc.py): the small per-segment host arrays of one launch
// packed into ONE pinned staging block (16-byte aligned sub-arrays), copied with ONE
// non-blocking H2D on the current stream, returned as typed device views.  Both blocks come
// from PyTorch's caching allocators (the pinned block is recorded on the copy's stream, so
// reuse waits for the copy).  In C++ the per-array work is a memcpy and a view: ~8 us per
// launch instead of ~19 us for the same steps in Python.
std::vector<Tensor> pack_h2d(const std::vector<pybind11::array>& arrays, int64_t device_index) {
  namespace py = pybind11;
  std::vector<py::array> arr;  // kept until their bytes are in the pinned block
  std::vector<int64_t> offs;
  std::vector<c10::ScalarType> types;
  int64_t total = 0;
  for (const auto& a0 : arrays) {
    py::array a = py::array::ensure(a0, py::array::c_style);
    TORCH_CHECK(a, "pack_h2d: not an array");
    const auto dt = a.dtype();
    const char kind = dt.kind();
    const auto size = dt.itemsize();
    c10::ScalarType st;
    if ((kind == 'i' || kind == 'u') && size == 8) st = torch::kInt64;
    else if ((kind == 'i' || kind == 'u') && size == 4) st = torch::kInt32;  // uint32 as int32 bits
    else if (kind == 'u' && size == 1) st = torch::kUInt8;
    else if (kind == 'i' && size == 1) st = torch::kInt8;
    else if (kind == 'f' && size == 8) st = torch::kFloat64;
    else TORCH_CHECK(false, "pack_h2d: unsupported dtype");
    offs.push_back(total);
    types.push_back(st);
    total += hlsp2p::host::Staging::aligned(static_cast<int64_t>(a.nbytes()));
    arr.push_back(std::move(a));
  }
  if (total < 16) total = 16;
  Tensor host = hlsp2p::host::pinned_bytes(total);
  uint8_t* h = host.data_ptr<uint8_t>();
  for (size_t i = 0; i < arr.size(); ++i)
    if (arr[i].nbytes()) std::memcpy(h + offs[i], arr[i].data(), arr[i].nbytes());
  Tensor dev = torch::empty({total}, torch::TensorOptions().dtype(torch::kUInt8).device(torch::kCUDA, device_index));
  dev.copy_(host, /*non_blocking=*/true);
  std::vector<Tensor> out;
  out.reserve(arr.size());
  for (size_t i = 0; i < arr.size(); ++i)
    out.push_back(dev.narrow(0, offs[i], static_cast<int64_t>(arr[i].nbytes())).view(types[i]));
  return out;
}

}  // namespace

// The same launches registered with the PyTorch dispatcher: torch.ops.hlsp2p.<name> (CUDA
// key, which is HIP on ROCm).  Each op writes its outputs in place (schemas mark them
// mutable) on the current stream, exactly like the pybind entry points above.  The
// dispatcher path lets torch-level code (custom autograd-free pipelines, torch.library
// tooling, opcheck) call the gfx950 kernels without this module's Python wrappers.
TORCH_LIBRARY(hlsp2p, m) {
  m.def("aes128_cbc_decrypt(Tensor src, Tensor(a!) dst, Tensor src_off, Tensor dst_off, Tensor blk_prefix, "
        "Tensor chunk_prefix, Tensor drk, Tensor iv, Tensor td0, Tensor isb, Tensor(b!) out_len, "
        "int total_chunks) -> ()");
  m.def("crc32_batch(Tensor buf, Tensor seg_off, Tensor seg_len, Tensor tile_prefix, Tensor res_off, Tensor wfrag, "
        "Tensor tables, Tensor(a!) residues, Tensor(b!) crc_out, Tensor? expect, Tensor(c!)? ok_out, "
        "int total_tiles, Tensor? scatter_idx, Tensor(d!)? scatter_out) -> ()");
  m.def("ts_demux(Tensor buf, Tensor seg_off, Tensor seg_len, Tensor blk_prefix, int total_blocks, "
        "Tensor(a!) meta, Tensor(b!) pts_dts, Tensor(c!) blk_sums, Tensor(d!) es, Tensor es_off, Tensor(e!) pes, "
        "int max_pes, Tensor(f!) info) -> ()");
  m.def("es_index(Tensor es, Tensor es_off, Tensor cap, Tensor tile_prefix, int total_tiles, Tensor info, Tensor pes, "
        "int max_pes, int max_nal, Tensor(a!) scratch, Tensor(b!) nal, Tensor(c!) au, Tensor(d!) aframes, "
        "Tensor(e!) sinfo) -> ()");
  m.def("remux(Tensor es, Tensor es_off, Tensor cap, Tensor tile_prefix, int total_tiles, Tensor info, Tensor pes, "
        "int max_pes, int max_nal, Tensor nal, Tensor au, Tensor aframes, Tensor sinfo, int max_aframes, "
        "Tensor(a!) scratch, Tensor(b!) vsamples, Tensor(c!) asamples, Tensor(d!) rinfo, Tensor(e!) out, "
        "Tensor out_off, int audio_gap=0) -> ()");
  m.def("fragment_moof(Tensor rinfo, Tensor vsamples, Tensor asamples, Tensor sinfo, Tensor fparams, int max_pes, "
        "int max_aframes, int headroom, int audio_gap, Tensor(a!) out, Tensor(b!) finfo, Tensor? mpainfo=None) -> ()");
  m.def("mpeg_audio(Tensor es, Tensor es_off, Tensor cap, Tensor tile_prefix, int total_tiles, Tensor info, Tensor pes, "
        "int max_pes, Tensor region, int max_aframes, Tensor(a!) scratch, Tensor(b!) mframes, Tensor(c!) mpainfo, "
        "Tensor(d!) asamples, Tensor(e!) rinfo, Tensor(f!) out, Tensor out_off) -> ()");
  m.def("ac3_audio(Tensor es, Tensor es_off, Tensor cap, Tensor tile_prefix, int total_tiles, Tensor info, Tensor pes, "
        "int max_pes, Tensor region, int max_aframes, Tensor(a!) scratch, Tensor(b!) dframes, Tensor(c!) ac3info, "
        "Tensor(d!) mpainfo, Tensor(e!) asamples, Tensor(f!) rinfo, Tensor(g!) out, Tensor out_off, "
        "Tensor? mpa_in=None) -> ()");
  m.def("codec_config(Tensor es, Tensor es_off, Tensor cap, Tensor info, Tensor pes, int max_pes, int max_nal, "
        "Tensor nal, Tensor au, Tensor aframes, Tensor sinfo, int max_ps, Tensor(a!) cinfo, Tensor(b!) ps) -> ()");
  m.def("hevc_config(Tensor es, Tensor es_off, Tensor cap, Tensor info, Tensor pes, int max_pes, int max_nal, "
        "Tensor nal, Tensor au, Tensor aframes, Tensor sinfo, int max_ps, Tensor(a!) hinfo, Tensor(b!) hps) -> ()");
  m.def("sample_aes_decrypt(Tensor(a!) es, Tensor es_off, Tensor cap, Tensor info, Tensor pes, int max_pes, "
        "int max_nal, Tensor(b!) nal, Tensor au, Tensor aframes, Tensor sinfo, Tensor round_keys, Tensor iv, "
        "Tensor enable, Tensor td, Tensor isb, Tensor(c!) sainfo) -> ()");
  m.def("cc_extract(Tensor es, Tensor es_off, Tensor cap, Tensor info, Tensor pes, int max_pes, int max_nal, "
        "Tensor nal, Tensor au, Tensor aframes, Tensor sinfo, Tensor enable, int max_cc, Tensor(a!) scratch, "
        "Tensor(b!) ccsamples, Tensor(c!) ccpts, Tensor(d!) ccbytes, Tensor(e!) cc608, Tensor(f!) ccinfo) -> ()");
  m.def("mp4_demux(Tensor buf, Tensor off, Tensor len, Tensor cap, Tensor tracks, int max_pes, int max_nal, "
        "int max_moof, int max_run, int max_emsg, Tensor(a!) minfo, Tensor(b!) msamples, Tensor(c!) runs, "
        "Tensor(d!) emsg, Tensor(e!) info, Tensor(f!) pes, Tensor(g!) nal, Tensor(h!) au, Tensor(i!) aframes, "
        "Tensor(j!) sinfo) -> ()");
  m.def("packed_audio(Tensor buf, Tensor off, Tensor len, Tensor cap, int max_pes, Tensor(a!) info, Tensor(b!) pes, "
        "Tensor(c!) nal, Tensor(d!) au, Tensor(e!) aframes, Tensor(f!) sinfo, Tensor(g!) painfo, "
        "bool staged=True) -> ()");
  m.def("cbcs_decrypt(Tensor src, Tensor src_off, Tensor cap, Tensor(a!) dst, Tensor dst_off, Tensor info, Tensor pes, "
        "Tensor minfo, Tensor msamples, Tensor runs, int max_pes, int max_run, Tensor prot, Tensor const_iv, Tensor iv, "
        "Tensor round_keys, Tensor enable, Tensor td, Tensor isb, int max_range, int max_blocks, Tensor(b!) scratch, "
        "Tensor(c!) ranges, Tensor(d!) cinfo) -> ()");
  m.def("cenc_decrypt(Tensor src, Tensor src_off, Tensor cap, Tensor(a!) dst, Tensor dst_off, Tensor info, Tensor pes, "
        "Tensor minfo, Tensor msamples, Tensor runs, int max_pes, int max_run, Tensor prot, Tensor const_iv, Tensor iv, "
        "Tensor round_keys, Tensor enable, Tensor te, Tensor sbox, int max_range, int max_cap, Tensor(b!) scratch, "
        "Tensor(c!) ranges, Tensor(d!) cinfo) -> ()");
  m.def("segment_copy(Tensor src, Tensor(a!) dst, Tensor src_off, Tensor dst_off, Tensor len, Tensor chunk_prefix, "
        "int total_chunks) -> ()");
}

TORCH_LIBRARY_IMPL(hlsp2p, CUDA, m) {
  m.impl("aes128_cbc_decrypt", &aes128_cbc_decrypt);
  m.impl("crc32_batch", &crc32_batch);
  m.impl("ts_demux", &ts_demux);
  m.impl("es_index", &es_index);
  m.impl("remux", &remux);
  m.impl("fragment_moof", &fragment_moof);
  m.impl("mpeg_audio", &mpeg_audio);
  m.impl("ac3_audio", &ac3_audio);
  m.impl("codec_config", &codec_config);
  m.impl("hevc_config", &hevc_config);
  m.impl("sample_aes_decrypt", &sample_aes_decrypt);
  m.impl("cc_extract", &cc_extract);
  m.impl("mp4_demux", &mp4_demux);
  m.impl("packed_audio", &packed_audio);
  m.impl("cbcs_decrypt", &cbcs_decrypt);
  m.impl("cenc_decrypt", &cenc_decrypt);
  m.impl("segment_copy", &segment_copy);
}

void register_rccl(pybind11::module& m);      // rccl_comm.cpp: native RCCL data plane
void register_transmux(pybind11::module& m);  // transmux.cpp: one native call per transmux batch
void register_ingest(pybind11::module& m);    // ingest.cpp: CRC launch + arena views for the node

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.doc() = "hlsjs-p2p-wrapper-amd CDNA4 (gfx950) kernels";
  m.def("aes128_cbc_decrypt", &aes128_cbc_decrypt);
  m.def("aes_chunk_blocks", &D::aes_chunk_blocks);
  namespace py = pybind11;
  m.def("crc32_batch", &crc32_batch, py::arg("buf"), py::arg("seg_off"), py::arg("seg_len"), py::arg("tile_prefix"),
        py::arg("res_off"), py::arg("wfrag"), py::arg("tables"), py::arg("residues"), py::arg("crc_out"),
        py::arg("expect"), py::arg("ok_out"), py::arg("total_tiles"), py::arg("scatter_idx") = py::none(),
        py::arg("scatter_out") = py::none());
  m.def("ts_demux", &ts_demux);
  m.def("es_index", &es_index);
  m.def("es_index_tile_bytes", &D::es_index_tile_bytes);
  m.def("ts_demux_blocks", py::vectorize(&ts::demux_blocks), py::arg("cap"));  // scalar or int64 array
  m.def("ts_demux_workspace", [](int64_t total_blocks, int64_t nseg) {
    const auto ws = ts::demux_workspace(total_blocks, nseg);
    return py::make_tuple(ws.meta, ws.pts_dts, ws.aux);
  }, py::arg("total_blocks"), py::arg("nseg"));
  m.def("es_index_scratch_words", [](int64_t total_tiles, int64_t nseg, int64_t max_nal) {
    return es_::index_scratch(total_tiles, nseg, max_nal).end;
  }, py::arg("total_tiles"), py::arg("nseg"), py::arg("max_nal"));
  m.def("remux", &remux, py::arg("es"), py::arg("es_off"), py::arg("cap"), py::arg("tile_prefix"),
        py::arg("total_tiles"), py::arg("info"), py::arg("pes"), py::arg("max_pes"), py::arg("max_nal"), py::arg("nal"),
        py::arg("au"), py::arg("aframes"), py::arg("sinfo"), py::arg("max_aframes"), py::arg("scratch"),
        py::arg("vsamples"), py::arg("asamples"), py::arg("rinfo"), py::arg("out"), py::arg("out_off"),
        py::arg("audio_gap") = 0);
  m.def("remux_tile_bytes", &D::remux_tile_bytes);
  m.def("remux_out_bytes", py::vectorize(&es_::remux_out_bytes), py::arg("cap"), py::arg("max_nal"));
  m.def("remux_scratch_words", [](int64_t nseg, int64_t max_nal, int64_t max_aframes) {
    return es_::remux_scratch(nseg, max_nal, max_aframes).end;
  }, py::arg("nseg"), py::arg("max_nal"), py::arg("max_aframes"));
  m.def("fragment_moof", &fragment_moof, py::arg("rinfo"), py::arg("vsamples"), py::arg("asamples"), py::arg("sinfo"),
        py::arg("fparams"), py::arg("max_pes"), py::arg("max_aframes"), py::arg("headroom"), py::arg("audio_gap"),
        py::arg("out"), py::arg("finfo"), py::arg("mpainfo") = py::none());
  m.def("mpeg_audio", &mpeg_audio);
  m.def("mpeg_audio_tile_bytes", &D::mpeg_audio_tile_bytes);
  m.def("mpa_scratch_words", [](int64_t nseg, int64_t max_pes) { return es_::mpa_scratch(nseg, max_pes).end; },
        py::arg("nseg"), py::arg("max_pes"));
  m.def("ac3_audio", &ac3_audio, py::arg("es"), py::arg("es_off"), py::arg("cap"), py::arg("tile_prefix"),
        py::arg("total_tiles"), py::arg("info"), py::arg("pes"), py::arg("max_pes"), py::arg("region"),
        py::arg("max_aframes"), py::arg("scratch"), py::arg("dframes"), py::arg("ac3info"), py::arg("mpainfo"),
        py::arg("asamples"), py::arg("rinfo"), py::arg("out"), py::arg("out_off"), py::arg("mpa_in") = py::none());
  m.def("ac3_audio_tile_bytes", &D::ac3_audio_tile_bytes);
  m.def("codec_config", &codec_config);
  m.def("hevc_config", &hevc_config);
  m.def("sample_aes_decrypt", &sample_aes_decrypt);
  m.def("sample_aes_round_bytes", &D::sample_aes_round_bytes);
  m.def("cc_extract", &cc_extract);
  m.def("cc_scratch_words", [](int64_t nseg, int64_t max_nal) { return es_::cc_scratch(nseg, max_nal).end; },
        py::arg("nseg"), py::arg("max_nal"));
  m.def("mp4_demux", &mp4_demux);
  m.def("packed_audio", &packed_audio, py::arg("buf"), py::arg("off"), py::arg("len"), py::arg("cap"), py::arg("max_pes"),
        py::arg("info"), py::arg("pes"), py::arg("nal"), py::arg("au"), py::arg("aframes"), py::arg("sinfo"),
        py::arg("painfo"), py::arg("staged") = true);
  m.def("packed_audio_tile_bytes", &D::packed_audio_tile_bytes);
  m.attr("CRC_GROUP_BYTES") = crc::kGroupBytes;
  m.attr("CRC_TILE_GROUPS") = crc::kTileGroups;
  m.def("cbcs_decrypt", &cbcs_decrypt);
  m.def("cenc_decrypt", &cenc_decrypt);
  m.def("segment_copy", &segment_copy);
  m.def("device_cus", &device_cus);
  m.def("h2d_batch", &h2d_batch, pybind11::arg("dst"), pybind11::arg("dst_off"), pybind11::arg("src_ptr"),
        pybind11::arg("len"), pybind11::arg("src_alloc"), pybind11::arg("max_gap"),
        pybind11::arg("device_src") = false);
  m.def("pack_h2d", &pack_h2d);
  register_rccl(m);
  register_transmux(m);
  register_ingest(m);
  m.attr("ARCH") = "gfx950";
}
