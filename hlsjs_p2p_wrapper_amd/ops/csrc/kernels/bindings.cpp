// torch binding module `_C`: argument checking + current-HIP-stream launch of the gfx950
// kernels, as pybind functions and as dispatcher ops (torch.ops.hlsp2p.*).  Host-only
// translation unit; kernels live in *.hip objects.
#include <c10/hip/HIPStream.h>
#include <hip/hip_runtime_api.h>
#include <torch/extension.h>
#include <pybind11/numpy.h>
#include <pybind11/stl.h>

#include <cstring>

namespace hlsp2p {
namespace dev {
int aes_chunk_blocks();
hipError_t launch_aes128_cbc_decrypt(const uint8_t*, uint8_t*, const int64_t*, const int64_t*, const int64_t*,
                                     const int64_t*, const uint32_t*, const uint32_t*, const uint32_t*,
                                     const uint8_t*, int64_t*, int, int64_t, int, hipStream_t, const int64_t*,
                                     const void*, uint32_t*, const int64_t*, void*);
hipError_t launch_crc32_batch(const uint8_t*, const int64_t*, const int64_t*, const int64_t*, const int64_t*,
                              const void*, const uint32_t*, uint32_t*, uint32_t*, const uint32_t*, uint8_t*,
                              const int64_t*, uint32_t*, int64_t, int, int64_t, int, bool, hipStream_t,
                              const int64_t*);
hipError_t launch_ts_demux(const uint8_t*, const int64_t*, const int64_t*, const int64_t*, int, int64_t, uint32_t*,
                           int64_t*, int32_t*, uint8_t*, const int64_t*, int64_t*, int64_t, int64_t*, hipStream_t,
                           const void*, const int64_t*);
int es_index_tile_bytes();
hipError_t launch_es_index(const uint8_t*, int64_t, const int64_t*, const int64_t*, const int64_t*, int, int64_t,
                           const int64_t*, const int64_t*, int64_t, int64_t, int32_t*, int32_t*, int32_t*, int32_t*,
                           int64_t*, hipStream_t);
hipError_t launch_segment_copy(const uint8_t*, uint8_t*, const int64_t*, const int64_t*, const int64_t*,
                               const int64_t*, int, int64_t, hipStream_t);
}  // namespace dev
}  // namespace hlsp2p

namespace {

using torch::Tensor;
namespace D = hlsp2p::dev;

void check(const Tensor& t, const char* name, c10::ScalarType dt, int64_t min_numel = 0) {
  TORCH_CHECK(t.is_cuda(), name, " must be a GPU tensor");
  TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
  TORCH_CHECK(t.scalar_type() == dt, name, " has dtype ", t.scalar_type(), ", expected ", dt);
  TORCH_CHECK(t.numel() >= min_numel, name, " too small: ", t.numel(), " < ", min_numel);
}

void same_device(const Tensor& a, const Tensor& b) {
  TORCH_CHECK(a.device() == b.device(), "tensors on different devices");
}

hipStream_t stream() { return c10::hip::getCurrentHIPStream().stream(); }

void ok(hipError_t e, const char* what) {
  TORCH_CHECK(e == hipSuccess, what, " launch failed: ", hipGetErrorString(e));
}

int num_cus(const Tensor& t) {
  static int cached[64] = {0};
  const int dev = t.get_device();
  if (dev >= 0 && dev < 64 && cached[dev]) return cached[dev];
  int n = 0;
  hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev);
  if (n <= 0) n = 256;
  if (dev >= 0 && dev < 64) cached[dev] = n;
  return n;
}

template <typename T>
const T* cptr(const Tensor& t) { return reinterpret_cast<const T*>(t.data_ptr()); }
template <typename T>
T* mptr(const Tensor& t) { return reinterpret_cast<T*>(t.data_ptr()); }

void aes128_cbc_decrypt(Tensor src, Tensor dst, Tensor src_off, Tensor dst_off, Tensor blk_prefix,
                        Tensor chunk_prefix, Tensor drk, Tensor iv, Tensor td0, Tensor isb, Tensor out_len,
                        int64_t total_chunks) {
  const int64_t B = src_off.numel();
  check(src, "src", torch::kUInt8);
  check(dst, "dst", torch::kUInt8);
  check(src_off, "src_off", torch::kInt64);
  check(dst_off, "dst_off", torch::kInt64, B);
  check(blk_prefix, "blk_prefix", torch::kInt64, B + 1);
  check(chunk_prefix, "chunk_prefix", torch::kInt64, B + 1);
  check(drk, "drk", torch::kInt32, B * 44);
  check(iv, "iv", torch::kUInt8, B * 16);
  check(td0, "td0", torch::kInt32, 256);
  check(isb, "isb", torch::kUInt8, 256);
  check(out_len, "out_len", torch::kInt64, B);
  TORCH_CHECK(src.data_ptr() != dst.data_ptr(), "CBC decrypt cannot run in place");
  TORCH_CHECK((reinterpret_cast<uintptr_t>(src.data_ptr()) & 15) == 0 &&
                  (reinterpret_cast<uintptr_t>(dst.data_ptr()) & 15) == 0,
              "src/dst must be 16-byte aligned");
  same_device(src, dst);
  ok(D::launch_aes128_cbc_decrypt(cptr<uint8_t>(src), mptr<uint8_t>(dst), cptr<int64_t>(src_off),
                                  cptr<int64_t>(dst_off), cptr<int64_t>(blk_prefix), cptr<int64_t>(chunk_prefix),
                                  cptr<uint32_t>(drk), cptr<uint32_t>(iv), cptr<uint32_t>(td0), cptr<uint8_t>(isb),
                                  mptr<int64_t>(out_len), static_cast<int>(B), total_chunks, num_cus(src), stream(),
                                  nullptr, nullptr, nullptr, nullptr, nullptr),
     "aes128_cbc_decrypt");
}

void crc32_batch(Tensor buf, Tensor seg_off, Tensor seg_len, Tensor tile_prefix, Tensor res_off, Tensor wfrag,
                 Tensor tables, Tensor residues, Tensor crc_out, c10::optional<Tensor> expect,
                 c10::optional<Tensor> ok_out, int64_t total_tiles, c10::optional<Tensor> scatter_idx,
                 c10::optional<Tensor> scatter_out) {
  const int64_t B = seg_off.numel();
  check(buf, "buf", torch::kUInt8);
  check(seg_off, "seg_off", torch::kInt64);
  check(seg_len, "seg_len", torch::kInt64, B);
  check(tile_prefix, "tile_prefix", torch::kInt64, B + 1);
  check(res_off, "res_off", torch::kInt64, B);
  // B fragments pick the matrix-core path: int8 [64 steps][64 lanes][16] for the i8 MFMA,
  // uint8 [32][64][16] of packed e2m1 nibbles for the FP4 f8f6f4 MFMA
  const bool fp4 = wfrag.scalar_type() == torch::kUInt8;
  check(wfrag, "wfrag", fp4 ? torch::kUInt8 : torch::kInt8, fp4 ? 32 * 64 * 16 : 64 * 64 * 16);
  check(tables, "tables", torch::kInt32, 48 * 1024);
  check(residues, "residues", torch::kInt32);
  check(crc_out, "crc_out", torch::kInt32, B);
  TORCH_CHECK((reinterpret_cast<uintptr_t>(buf.data_ptr()) & 15) == 0, "buf must be 16-byte aligned");
  const uint32_t* ex = nullptr;
  uint8_t* okp = nullptr;
  if (expect.has_value()) {
    check(*expect, "expect", torch::kInt32, B);
    ex = cptr<uint32_t>(*expect);
  }
  if (ok_out.has_value()) {
    check(*ok_out, "ok_out", torch::kUInt8, B);
    okp = mptr<uint8_t>(*ok_out);
  }
  const int64_t* sidx = nullptr;
  uint32_t* sout = nullptr;
  int64_t sn = 0;
  TORCH_CHECK(scatter_idx.has_value() == scatter_out.has_value(), "scatter_idx and scatter_out go together");
  if (scatter_out.has_value()) {
    check(*scatter_idx, "scatter_idx", torch::kInt64, B);
    check(*scatter_out, "scatter_out", torch::kInt32);
    sidx = cptr<int64_t>(*scatter_idx);
    sout = mptr<uint32_t>(*scatter_out);
    sn = scatter_out->numel();
  }
  ok(D::launch_crc32_batch(cptr<uint8_t>(buf), cptr<int64_t>(seg_off), cptr<int64_t>(seg_len),
                           cptr<int64_t>(tile_prefix), cptr<int64_t>(res_off), wfrag.data_ptr(),
                           cptr<uint32_t>(tables), mptr<uint32_t>(residues), mptr<uint32_t>(crc_out), ex, okp,
                           sidx, sout, sn, static_cast<int>(B), total_tiles, num_cus(buf), fp4, stream(), nullptr),
     "crc32_batch");
}

void ts_demux(Tensor buf, Tensor seg_off, Tensor seg_len, Tensor blk_prefix, int64_t total_blocks, Tensor meta,
              Tensor pts_dts, Tensor blk_sums, Tensor es, Tensor es_off, Tensor pes, int64_t max_pes, Tensor info) {
  const int64_t B = seg_off.numel();
  check(buf, "buf", torch::kUInt8);
  check(seg_off, "seg_off", torch::kInt64);
  check(seg_len, "seg_len", torch::kInt64, B);
  check(blk_prefix, "blk_prefix", torch::kInt64, B + 1);
  check(meta, "meta", torch::kInt32, total_blocks * 256);
  check(pts_dts, "pts_dts", torch::kInt64, total_blocks * 256 * 2);
  check(blk_sums, "aux", torch::kInt32, total_blocks * 12 + B * 7);  // sums | prefixes | totals | counters
  check(es, "es", torch::kUInt8);
  check(es_off, "es_off", torch::kInt64, B);
  check(pes, "pes", torch::kInt64, B * 3 * max_pes * 3);
  check(info, "info", torch::kInt64, B * 24);
  TORCH_CHECK((reinterpret_cast<uintptr_t>(buf.data_ptr()) & 15) == 0, "buf must be 16-byte aligned");
  ok(D::launch_ts_demux(cptr<uint8_t>(buf), cptr<int64_t>(seg_off), cptr<int64_t>(seg_len),
                        cptr<int64_t>(blk_prefix), static_cast<int>(B), total_blocks, mptr<uint32_t>(meta),
                        mptr<int64_t>(pts_dts), mptr<int32_t>(blk_sums), mptr<uint8_t>(es), cptr<int64_t>(es_off),
                        mptr<int64_t>(pes), max_pes, mptr<int64_t>(info), stream(), nullptr, nullptr),
     "ts_demux");
}

// Sample index of a demuxed batch (es_index.hip): es / info / pes are ts_demux's outputs, cap the
// host upper bound of each segment's ES bytes (the Python wrapper has checked es_off + cap
// against es), tile_prefix the exclusive prefix of ceil(cap / es_index_tile_bytes()).
void es_index(Tensor es, Tensor es_off, Tensor cap, Tensor tile_prefix, int64_t total_tiles, Tensor info, Tensor pes,
              int64_t max_pes, int64_t max_nal, Tensor scratch, Tensor nal, Tensor au, Tensor aframes, Tensor sinfo) {
  const int64_t B = es_off.numel();
  TORCH_CHECK(max_pes > 0 && max_nal > 0 && total_tiles >= 0, "es_index: max_pes / max_nal / total_tiles out of range");
  check(es, "es", torch::kUInt8);
  check(es_off, "es_off", torch::kInt64);
  check(cap, "cap", torch::kInt64, B);
  check(tile_prefix, "tile_prefix", torch::kInt64, B + 1);
  check(info, "info", torch::kInt64, B * 24);
  check(pes, "pes", torch::kInt64, B * 3 * max_pes * 3);
  check(scratch, "scratch", torch::kInt32, 2 * total_tiles + B * (max_nal + 1));  // counts | prefixes | positions
  check(nal, "nal", torch::kInt32, B * max_nal * 4);
  check(au, "au", torch::kInt32, B * max_pes * 4);
  check(aframes, "aframes", torch::kInt32, B * max_pes * 2);
  check(sinfo, "sinfo", torch::kInt64, B * 8);
  same_device(es, sinfo);
  TORCH_CHECK((reinterpret_cast<uintptr_t>(es.data_ptr()) & 15) == 0, "es must be 16-byte aligned");
  ok(D::launch_es_index(cptr<uint8_t>(es), es.numel(), cptr<int64_t>(es_off), cptr<int64_t>(cap),
                        cptr<int64_t>(tile_prefix), static_cast<int>(B), total_tiles, cptr<int64_t>(info),
                        cptr<int64_t>(pes), max_pes, max_nal, mptr<int32_t>(scratch), mptr<int32_t>(nal),
                        mptr<int32_t>(au), mptr<int32_t>(aframes), mptr<int64_t>(sinfo), stream()),
     "es_index");
}

void segment_copy(Tensor src, Tensor dst, Tensor src_off, Tensor dst_off, Tensor len, Tensor chunk_prefix,
                  int64_t total_chunks) {
  const int64_t n = src_off.numel();
  check(src, "src", torch::kUInt8);
  check(dst, "dst", torch::kUInt8);
  check(src_off, "src_off", torch::kInt64);
  check(dst_off, "dst_off", torch::kInt64, n);
  check(len, "len", torch::kInt64, n);
  check(chunk_prefix, "chunk_prefix", torch::kInt64, n + 1);
  ok(D::launch_segment_copy(cptr<uint8_t>(src), mptr<uint8_t>(dst), cptr<int64_t>(src_off), cptr<int64_t>(dst_off),
                            cptr<int64_t>(len), cptr<int64_t>(chunk_prefix), static_cast<int>(n), total_chunks,
                            stream()),
     "segment_copy");
}

int64_t device_cus(Tensor t) { return num_cus(t); }

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
  check(dst, "dst", torch::kUInt8);
  const int64_t n = dst_off.size();
  TORCH_CHECK(src_ptr.size() == n && len.size() == n && src_alloc.size() == n, "h2d_batch: argument sizes differ");
  const int64_t* o = dst_off.data();
  const int64_t* s = src_ptr.data();
  const int64_t* l = len.data();
  const int64_t* a = src_alloc.data();
  uint8_t* base = mptr<uint8_t>(dst);
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
    ok(hipMemcpyAsync(base + o[i], reinterpret_cast<const void*>(s[i]), static_cast<size_t>(bytes),
                      device_src ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st),
       "hipMemcpyAsync");
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
  std::vector<py::array> arr;
  arr.reserve(arrays.size());
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
    total += (static_cast<int64_t>(a.nbytes()) + 15) & ~int64_t(15);
    arr.push_back(std::move(a));
  }
  if (total < 16) total = 16;
  Tensor host = torch::empty({total}, torch::TensorOptions().dtype(torch::kUInt8).pinned_memory(true));
  uint8_t* h = host.data_ptr<uint8_t>();
  for (size_t i = 0; i < arr.size(); ++i) std::memcpy(h + offs[i], arr[i].data(), arr[i].nbytes());
  Tensor dev = torch::empty({total}, torch::TensorOptions().dtype(torch::kUInt8).device(torch::kCUDA, device_index));
  dev.copy_(host, /*non_blocking=*/true);
  std::vector<Tensor> out;
  out.reserve(arr.size());
  for (size_t i = 0; i < arr.size(); ++i) {
    const int64_t nb = static_cast<int64_t>(arr[i].nbytes());
    out.push_back(dev.narrow(0, offs[i], nb).view(types[i]));
  }
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
  m.def("segment_copy(Tensor src, Tensor(a!) dst, Tensor src_off, Tensor dst_off, Tensor len, Tensor chunk_prefix, "
        "int total_chunks) -> ()");
}

TORCH_LIBRARY_IMPL(hlsp2p, CUDA, m) {
  m.impl("aes128_cbc_decrypt", &aes128_cbc_decrypt);
  m.impl("crc32_batch", &crc32_batch);
  m.impl("ts_demux", &ts_demux);
  m.impl("es_index", &es_index);
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
