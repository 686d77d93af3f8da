// pybind11 module `_runtime`: the host-native runtime of the swarm node.
//
// Pure C++ (no torch, no HIP): cache layout + swarm directory + exchange planner, the
// origin packager (TS mux + AES-128-CBC), and CPU reference implementations of every
// device kernel (decrypt, demux, CRC) used as test oracles and by the CPU (no-GPU) mode.
// Batch entry points take numpy arrays (torch CPU tensors pass via .numpy()).
#include <pybind11/numpy.h>
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include <algorithm>
#include <cstring>
#include <initializer_list>
#include <map>
#include <optional>
#include <sstream>
#include <stdexcept>
#include <thread>
#include <tuple>
#include <type_traits>
#include <vector>

#include "aes_host.hpp"
#include "captions.hpp"
#include "cbcs.hpp"
#include "cenc.hpp"
#include "codec.hpp"
#include "crc_host.hpp"
#include "es.hpp"
#include "fragment.hpp"
#include "hevc.hpp"
#include "locator.hpp"
#include "mp4.hpp"
#include "ac3audio.hpp"
#include "mpegaudio.hpp"
#include "packedaudio.hpp"
#include "planner.hpp"
#include "remux.hpp"
#include "sampleaes.hpp"
#include "shm_control.hpp"
#include "store.hpp"
#include "ts.hpp"
#include "wants.hpp"

namespace py = pybind11;
using namespace hlsp2p;

namespace {

template <typename T>
using Arr = py::array_t<T, py::array::c_style | py::array::forcecast>;

template <typename T>
T* mut_ptr(py::array& a, const char* name) {
  if (!(a.flags() & py::array::c_style)) throw std::invalid_argument(std::string(name) + " must be C-contiguous");
  if (a.itemsize() != sizeof(T)) throw std::invalid_argument(std::string(name) + " has the wrong dtype");
  if (!a.writeable()) throw std::invalid_argument(std::string(name) + " must be writeable");
  return static_cast<T*>(a.mutable_data());
}

template <typename F>
void parallel_for(int64_t n, F&& f, int64_t work_bytes = -1) {
  unsigned hw = std::max(1u, std::thread::hardware_concurrency());
  int64_t nt = std::min<int64_t>(n, std::min<unsigned>(hw, 16u));
  // a thread spawn costs ~10-20 us: small batches (host-path probes, unit tests) run inline
  if (work_bytes >= 0) nt = std::min<int64_t>(nt, std::max<int64_t>(1, work_bytes >> 20));
  if (nt <= 1) {
    for (int64_t i = 0; i < n; ++i) f(i);
    return;
  }
  std::vector<std::thread> th;
  for (int64_t t = 0; t < nt; ++t)
    th.emplace_back([&, t] {
      for (int64_t i = t; i < n; i += nt) f(i);
    });
  for (auto& x : th) x.join();
}

// The demuxed and indexed batch every op from index_batch to caption_batch takes: its sizes are
// checked here, once (`more_ok`: the caller's own sizes, part of the same check), then each
// segment's ES range and, right behind it, whatever `also(b)` checks of segment b.
struct EsBatch {
  const uint8_t* es;
  const int64_t *es_off, *cap, *info, *pes;
  int64_t max_pes, max_nal;
  int64_t total = 0;  // ES bytes, the work to spread over threads
  es::Segment at(int64_t b) const { return es::segment_at(es, es_off, cap, info, pes, max_pes, max_nal, b); }
};
template <typename F>
EsBatch es_batch(const std::string& op, const Arr<uint8_t>& es, const Arr<int64_t>& es_off, const Arr<int64_t>& cap,
                 const Arr<int64_t>& info, const Arr<int64_t>& pes, int64_t max_pes, int64_t max_nal,
                 const es::IndexTables<const py::array, const py::array>& ix, bool more_ok, F&& also) {
  const int64_t B = es_off.size();
  if (cap.size() != B || !more_ok || info.size() < B * ts::kInfoWords || pes.size() < ts::pes_words(B, max_pes) ||
      ix.nal->size() < table_words(B, max_nal, es::kNalWords) || ix.au->size() < table_words(B, max_pes, es::kAuWords) ||
      ix.aframes->size() < table_words(B, max_pes, es::kApesWords) || ix.sinfo->size() < B * es::kSinfoWords)
    throw std::invalid_argument(op + ": an argument is too small");
  EsBatch r{es.data(), es_off.data(), cap.data(), info.data(), pes.data(), max_pes, max_nal};
  for (int64_t b = 0; b < B; ++b) {
    if (r.es_off[b] < 0 || r.cap[b] < 0 || r.es_off[b] + r.cap[b] > es.size())
      throw std::invalid_argument(op + ": ES out of bounds");
    also(b);
    r.total += r.cap[b];
  }
  return r;
}

// A table's pointer as the op's es::IndexTables asks for it.  A table the op writes comes as a
// py::array and has to be writeable as it is; one it only reads comes as an Arr.  IndexTables has
// one I32 for nal, au and aframes, so sample_decrypt_batch, which rewrites nal alone, gets the two
// it only reads through `int32_t*` as well.
template <typename T>
T* table_ptr(py::array& a, const char* name) { return mut_ptr<T>(a, name); }
template <typename T>
T* table_ptr(const Arr<std::remove_const_t<T>>& a, const char*) { return const_cast<T*>(a.data()); }

// One op on a demuxed and indexed batch, whole: es_batch's checks (`sized`, `also` as there), then
// `body(segment b, its index tables, b)` for every segment, on threads and without the GIL.
// I32 / I64 as in es::IndexTables: const where the op only reads the table.
template <typename I32, typename I64, typename Nal, typename Rows, typename Sinfo, typename Also, typename Body>
void each_segment(const std::string& op, const Arr<uint8_t>& es, const Arr<int64_t>& es_off, const Arr<int64_t>& cap,
                  const Arr<int64_t>& info, const Arr<int64_t>& pes, int64_t max_pes, int64_t max_nal, Nal& nal,
                  Rows& au, Rows& aframes, Sinfo& sinfo, bool sized, Also&& also, Body&& body) {
  if (max_pes <= 0 || max_nal <= 0) throw std::invalid_argument(op + ": max_pes and max_nal must be positive");
  const es::IndexTables<I32, I64> ix{table_ptr<I32>(nal, "nal"), table_ptr<I32>(au, "au"),
                                     table_ptr<I32>(aframes, "aframes"), table_ptr<I64>(sinfo, "sinfo")};
  const EsBatch batch =
      es_batch(op, es, es_off, cap, info, pes, max_pes, max_nal, {&nal, &au, &aframes, &sinfo}, sized, also);
  py::gil_scoped_release nogil;
  parallel_for(es_off.size(), [&](int64_t b) {
    const es::Segment s = batch.at(b);
    body(s, es::index_tables_at(ix, s, b), b);
  }, batch.total);
}
const auto no_check = [](int64_t) {};

// One name dictionary of the module: slots or bits of a shared/layout.hpp enum by name, as Python ints.
struct Named {
  const char* name;
  int64_t value;
};
py::dict name_dict(py::module_& m, const char* attr, std::initializer_list<Named> items) {
  py::dict d;
  for (const Named& n : items) d[n.name] = n.value;
  m.attr(attr) = d;
  return d;
}

SegKey key_from(const int64_t* p) {
  return SegKey{uint32_t(p[0]), uint32_t(p[1]), uint32_t(p[2]), uint32_t(p[3])};
}

py::array_t<uint8_t> to_u8(const std::vector<uint8_t>& v) {
  py::array_t<uint8_t> a(static_cast<py::ssize_t>(v.size()));
  std::memcpy(a.mutable_data(), v.data(), v.size());
  return a;
}

}  // namespace

namespace {
// Replicated swarm state that differs across ranks (directory content or a round's plan).
struct SwarmDivergence : std::runtime_error {
  using std::runtime_error::runtime_error;
};

// "digest A: ranks [0, 1, 2]; digest B: ranks [3]" for one header word of every rank
std::string group_ranks(const std::vector<Arr<int64_t>>& parts, int64_t word) {
  std::map<int64_t, std::vector<int>> by;
  for (size_t r = 0; r < parts.size(); ++r) by[parts[r].data()[word]].push_back(int(r));
  std::ostringstream o;
  bool first = true;
  for (const auto& kv : by) {
    o << (first ? "" : "; ") << std::hex << "0x" << uint64_t(kv.first) << std::dec << ": ranks [";
    for (size_t i = 0; i < kv.second.size(); ++i) o << (i ? ", " : "") << kv.second[i];
    o << "]";
    first = false;
  }
  return o.str();
}
}  // namespace

PYBIND11_MODULE(_runtime, m) {
  py::register_exception<SwarmDivergence>(m, "SwarmDivergence", PyExc_RuntimeError);
  m.doc() = "hlsjs-p2p-wrapper-amd host runtime (store, planner, packager, CPU oracles)";

  // ------------------------------------------------------------------ AES
  m.def("aes_tables", [] {
    const aes::Tables& t = aes::tables();
    Arr<uint32_t> td0(256), te0(256);
    Arr<uint8_t> sbox(256), inv(256);
    std::memcpy(td0.mutable_data(), t.td0, sizeof t.td0);
    std::memcpy(te0.mutable_data(), t.te0, sizeof t.te0);
    std::memcpy(sbox.mutable_data(), t.sbox, 256);
    std::memcpy(inv.mutable_data(), t.inv_sbox, 256);
    return py::make_tuple(td0, inv, te0, sbox);
  });
  m.def("expand_key_dec", [](py::bytes key) {
    std::string k = key;
    if (k.size() != 16) throw std::invalid_argument("AES-128 key must be 16 bytes");
    Arr<uint32_t> out(44);
    aes::expand_key_dec(reinterpret_cast<const uint8_t*>(k.data()), out.mutable_data());
    return out;
  });
  m.def("expand_key_enc", [](py::bytes key) {
    std::string k = key;
    if (k.size() != 16) throw std::invalid_argument("AES-128 key must be 16 bytes");
    Arr<uint32_t> out(44);
    aes::expand_key_enc(reinterpret_cast<const uint8_t*>(k.data()), out.mutable_data());
    return out;
  });
  m.def("aes_encrypt_block", [](py::bytes key, py::bytes block) {
    std::string k = key, b = block;
    if (k.size() != 16 || b.size() != 16) throw std::invalid_argument("16-byte key and block");
    uint32_t rk[44];
    aes::expand_key_enc(reinterpret_cast<const uint8_t*>(k.data()), rk);
    uint8_t out[16];
    aes::encrypt_block(rk, reinterpret_cast<const uint8_t*>(b.data()), out);
    return py::bytes(reinterpret_cast<char*>(out), 16);
  });
  m.def("cbc_encrypt", [](py::bytes key, py::bytes iv, Arr<uint8_t> data) {
    std::string k = key, v = iv;
    if (k.size() != 16 || v.size() != 16) throw std::invalid_argument("16-byte key and iv");
    const size_t n = static_cast<size_t>(data.size());
    std::vector<uint8_t> out(n + 16);
    size_t total;
    {
      py::gil_scoped_release nogil;
      total = aes::cbc_encrypt_pkcs7(reinterpret_cast<const uint8_t*>(k.data()),
                                     reinterpret_cast<const uint8_t*>(v.data()), data.data(), n, out.data());
    }
    out.resize(total);
    return to_u8(out);
  });
  m.def("cbc_decrypt", [](py::bytes key, py::bytes iv, Arr<uint8_t> data) -> py::object {
    std::string k = key, v = iv;
    if (k.size() != 16 || v.size() != 16) throw std::invalid_argument("16-byte key and iv");
    const size_t n = static_cast<size_t>(data.size());
    std::vector<uint8_t> out(n);
    int64_t len;
    {
      py::gil_scoped_release nogil;
      len = aes::cbc_decrypt_pkcs7(reinterpret_cast<const uint8_t*>(k.data()),
                                   reinterpret_cast<const uint8_t*>(v.data()), data.data(), n, out.data());
    }
    if (len < 0) return py::none();
    out.resize(static_cast<size_t>(len));
    return to_u8(out);
  });
  // Batched CPU decrypt with the device kernel's argument layout.
  //   src/dst: flat uint8; src_off/dst_off/nbytes: int64[B]; drk: uint32[B,44]; iv: uint8[B,16]
  //   out_len: int64[B] (plaintext length after PKCS#7, -1 on bad padding)
  m.def("cbc_decrypt_batch", [](Arr<uint8_t> src, py::array dst, Arr<int64_t> src_off, Arr<int64_t> dst_off,
                                Arr<int64_t> nbytes, Arr<uint32_t> drk, Arr<uint8_t> iv, py::array out_len) {
    const int64_t B = src_off.size();
    uint8_t* d = mut_ptr<uint8_t>(dst, "dst");
    int64_t* ol = mut_ptr<int64_t>(out_len, "out_len");
    const uint8_t* s = src.data();
    const int64_t* so = src_off.data();
    const int64_t* dof = dst_off.data();
    const int64_t* nb = nbytes.data();
    const uint32_t* k = drk.data();
    const uint8_t* ivp = iv.data();
    const int64_t src_n = src.size(), dst_n = dst.size();
    for (int64_t b = 0; b < B; ++b)
      if (nb[b] < 0 || nb[b] % 16 || so[b] < 0 || so[b] + nb[b] > src_n || dof[b] < 0 || dof[b] + nb[b] > dst_n)
        throw std::invalid_argument("cbc_decrypt_batch: segment out of bounds or not a multiple of 16");
    int64_t total = 0;
    for (int64_t b = 0; b < B; ++b) total += nb[b];
    py::gil_scoped_release nogil;
    parallel_for(B, [&](int64_t b) {
      uint8_t* out = d + dof[b];
      aes::cbc_decrypt_raw(k + 44 * b, ivp + 16 * b, s + so[b], static_cast<size_t>(nb[b]), out);
      int64_t len = -1;
      if (nb[b] >= 16) {
        uint8_t pad = out[nb[b] - 1];
        if (pad >= 1 && pad <= 16) {
          len = nb[b] - pad;
          for (int64_t i = len; i < nb[b]; ++i)
            if (out[i] != pad) { len = -1; break; }
        }
      }
      ol[b] = len;
    }, total);
  });

  // ------------------------------------------------------------------ CRC
  m.def("crc32", [](Arr<uint8_t> data, uint32_t crc) {
    return crc::crc32(data.data(), static_cast<size_t>(data.size()), crc);
  }, py::arg("data"), py::arg("crc") = 0u);
  m.def("crc32_batch", [](Arr<uint8_t> buf, Arr<int64_t> off, Arr<int64_t> len) {
    const int64_t B = off.size();
    Arr<uint32_t> out(B);
    uint32_t* o = out.mutable_data();
    const uint8_t* p = buf.data();
    const int64_t* of = off.data();
    const int64_t* ln = len.data();
    for (int64_t b = 0; b < B; ++b)
      if (of[b] < 0 || ln[b] < 0 || of[b] + ln[b] > buf.size()) throw std::invalid_argument("crc32_batch: out of bounds");
    int64_t total = 0;
    for (int64_t b = 0; b < B; ++b) total += ln[b];
    py::gil_scoped_release nogil;
    parallel_for(B, [&](int64_t b) { o[b] = crc::crc32(p + of[b], static_cast<size_t>(ln[b])); }, total);
    return out;
  });
  m.def("crc_mfma_weights", [] {
    auto w = crc::mfma_group_weights();
    Arr<int8_t> a(static_cast<py::ssize_t>(w.size()));
    std::memcpy(a.mutable_data(), w.data(), w.size());
    return a;
  });
  m.def("crc_mfma_weights_fp4", [] {
    auto w = crc::mfma_group_weights_fp4();
    Arr<uint8_t> a(static_cast<py::ssize_t>(w.size()));
    std::memcpy(a.mutable_data(), w.data(), w.size());
    return a;
  });
  m.def("crc_chunk_weights_fp4", [] {
    auto w = crc::mfma_chunk_weights_fp4();
    Arr<uint8_t> a(static_cast<py::ssize_t>(w.size()));
    std::memcpy(a.mutable_data(), w.data(), w.size());
    return a;
  });
  m.def("crc_init_fold", &crc::init_fold, py::arg("nbytes"));
  m.def("crc_shift_tables", [] {
    auto t = crc::shift_tables();
    Arr<uint32_t> a(static_cast<py::ssize_t>(t.size()));
    std::memcpy(a.mutable_data(), t.data(), t.size() * 4);
    return a;
  });
  m.attr("CRC_NUM_P") = crc::kNumP;
  m.attr("CRC_NUM_Q") = crc::kNumQ;
  m.attr("CRC_GROUP_BYTES") = crc::kGroupBytes;
  m.attr("CRC_CHUNK_BYTES") = crc::kChunkBytes;
  m.attr("CRC_FUSED_AES_STEPS") = crc::kFusedAesSteps;
  m.attr("CRC_FUSED_FOLD_STEPS") = crc::kFusedFoldSteps;
  m.attr("CRC_FUSED_MASK_DWORDS") = crc::kFusedMaskDwords;

  // ------------------------------------------------------------------ TS
  m.def("mux_segment", [](double duration, double fps, int64_t target_bytes, int audio_kbps, bool with_id3,
                          uint64_t seed, int64_t sn, double start_time) {
    ts::MuxConfig c;
    c.duration = duration; c.fps = fps; c.target_bytes = target_bytes; c.audio_kbps = audio_kbps;
    c.with_id3 = with_id3; c.seed = seed; c.sn = sn; c.start_time = start_time;
    ts::MuxStats st;
    std::vector<uint8_t> v;
    {
      py::gil_scoped_release nogil;
      v = ts::mux_segment(c, &st);
    }
    py::dict d;
    d["es_bytes"] = py::make_tuple(st.es_bytes[0], st.es_bytes[1], st.es_bytes[2]);
    d["n_pes"] = py::make_tuple(st.n_pes[0], st.n_pes[1], st.n_pes[2]);
    d["first_pts"] = py::make_tuple(st.first_pts[0], st.first_pts[1], st.first_pts[2]);
    d["last_pts"] = py::make_tuple(st.last_pts[0], st.last_pts[1], st.last_pts[2]);
    d["n_packets"] = st.n_packets;
    return py::make_tuple(to_u8(v), d);
  }, py::arg("duration"), py::arg("fps"), py::arg("target_bytes"), py::arg("audio_kbps"), py::arg("with_id3"),
     py::arg("seed"), py::arg("sn"), py::arg("start_time"));
  // Batched CPU demux with the device kernels' layout.
  //   buf: flat uint8 plaintext; off/len: int64[B]; es: flat uint8 (segment b writes at es_off[b])
  //   pes: int64[B, TS_CLASSES, max_pes, TS_PES_WORDS]; info: int64[B, TS_INFO_WORDS]
  m.def("demux_batch", [](Arr<uint8_t> buf, Arr<int64_t> off, Arr<int64_t> len, py::array es, Arr<int64_t> es_off,
                          py::array pes, py::array info, int64_t max_pes) {
    const int64_t B = off.size();
    uint8_t* e = mut_ptr<uint8_t>(es, "es");
    int64_t* pp = mut_ptr<int64_t>(pes, "pes");
    int64_t* ip = mut_ptr<int64_t>(info, "info");
    if (pes.size() < ts::pes_words(B, max_pes) || info.size() < B * ts::kInfoWords)
      throw std::invalid_argument("demux_batch: pes/info too small");
    for (int64_t b = 0; b < B; ++b)
      if (off.data()[b] < 0 || len.data()[b] < 0 || off.data()[b] + len.data()[b] > buf.size() ||
          es_off.data()[b] < 0 || es_off.data()[b] + len.data()[b] > es.size())
        throw std::invalid_argument("demux_batch: segment out of bounds");
    const uint8_t* p = buf.data();
    const int64_t* o = off.data();
    const int64_t* l = len.data();
    const int64_t* eo = es_off.data();
    int64_t total = 0;
    for (int64_t b = 0; b < B; ++b) total += l[b];
    py::gil_scoped_release nogil;
    parallel_for(B, [&](int64_t b) {
      ts::demux_segment(p + o[b], l[b], e + eo[b], pp + ts::pes_words(b, max_pes), max_pes,
                        ip + b * ts::kInfoWords);
    }, total);
  });
  m.def("mpeg_crc32", [](Arr<uint8_t> data) { return ts::mpeg_crc32(data.data(), static_cast<size_t>(data.size())); });
  m.attr("TS_INFO_WORDS") = ts::kInfoWords;
  m.attr("TS_CLASSES") = ts::kClasses;
  m.attr("TS_PACKET") = ts::kPacket;
  m.attr("TS_PES_WORDS") = ts::kPesWords;
  {  // the info row and status bits by name (shared/layout.hpp)
    py::dict d = name_dict(m, "TS_INFO", {{"status", ts::kStatus}, {"pmt_pid", ts::kPmtPid},
                                          {"n_packets", ts::kNumPackets}, {"video_type", ts::kVideoType},
                                          {"audio_type", ts::kAudioType}, {"payload_bytes", ts::kPayloadBytes},
                                          {"audio_es_offset", ts::kAudioEsOffset},
                                          {"id3_es_offset", ts::kId3EsOffset}});
    const char* cls[ts::kClasses] = {"video", "audio", "id3"};
    for (int c = 0; c < ts::kClasses; ++c) {  // the per-class families: base slot + class
      const std::string n = cls[c];
      d[py::str(n + "_pid")] = ts::kVideoPid + c;
      d[py::str(n + "_bytes")] = ts::kVideoBytes + c;
      d[py::str("n_" + n + "_pes")] = ts::kNumVideoPes + c;
      d[py::str(n + "_first_pts")] = ts::kFirstPts + c;
      d[py::str(n + "_last_pts")] = ts::kLastPts + c;
    }
    name_dict(m, "TS_STATUS", {{"bad_sync", ts::kBadSync}, {"no_pat", ts::kNoPat}, {"no_pmt", ts::kNoPmt},
                               {"pes_overflow", ts::kPesOverflow}, {"pes_header_error", ts::kPesHeaderError},
                               {"bad_length", ts::kBadLength}});
  }
  // Batched CPU sample index with the device kernels' layout (docs/ESINDEX.md).
  //   es: flat uint8 (segment b's ES at es_off[b], cap[b] bytes readable); info / pes: demux_batch's
  //   nal: int32[B, max_nal, ES_NAL_WORDS]; au: int32[B, max_pes, ES_AU_WORDS];
  //   aframes: int32[B, max_pes, ES_APES_WORDS]; sinfo: int64[B, ES_SINFO_WORDS]
  m.def("index_batch", [](Arr<uint8_t> es, Arr<int64_t> es_off, Arr<int64_t> cap, Arr<int64_t> info, Arr<int64_t> pes,
                          int64_t max_pes, int64_t max_nal, py::array nal, py::array au, py::array aframes,
                          py::array sinfo) {
    each_segment<int32_t, int64_t>("index_batch", es, es_off, cap, info, pes, max_pes, max_nal, nal, au, aframes, sinfo,
                                   true, no_check, [](const es::Segment& s, const auto& out, int64_t) {
      es::index_segment(s, out);
    });
  });
  m.attr("ES_SINFO_WORDS") = es::kSinfoWords;
  m.attr("ES_NAL_WORDS") = es::kNalWords;
  m.attr("ES_AU_WORDS") = es::kAuWords;
  m.attr("ES_APES_WORDS") = es::kApesWords;
  m.attr("ES_DEFAULT_MAX_NAL") = es::kDefaultMaxNal;
  name_dict(m, "ES_SINFO", {{"status", es::kStatus}, {"n_nal", es::kNumNal}, {"n_au", es::kNumAu},
                            {"n_keyframe_aus", es::kNumKeyframeAus}, {"first_keyframe_au", es::kFirstKeyframeAu},
                            {"n_adts_frames", es::kNumAdtsFrames}, {"audio_sample_rate", es::kAudioSampleRate},
                            {"audio_channels", es::kAudioChannels}});
  name_dict(m, "ES_STATUS", {{"nal_overflow", es::kNalOverflow}, {"adts_error", es::kAdtsError},
                             {"unsupported_video", es::kUnsupportedVideo}});
  name_dict(m, "ES_AU_FLAGS", {{"keyframe", es::kAuKeyframe}, {"sps", es::kAuSps}, {"pps", es::kAuPps},
                               {"aud", es::kAuAud}});
  // Batched CPU remux with the device kernels' layout (docs/REMUX.md): the inputs of index_batch, its
  // four outputs, and per segment a region of remux_out_bytes(cap, max_nal) + audio_gap bytes of `out`
  // at out_off.
  //   vsamples: int32[B, max_pes, ES_VSAMPLE_WORDS]; asamples: int32[B, max_aframes, ES_ASAMPLE_WORDS];
  //   rinfo: int64[B, ES_RINFO_WORDS]
  m.def("remux_batch", [](Arr<uint8_t> es, Arr<int64_t> es_off, Arr<int64_t> cap, Arr<int64_t> info, Arr<int64_t> pes,
                          int64_t max_pes, int64_t max_nal, Arr<int32_t> nal, Arr<int32_t> au, Arr<int32_t> aframes,
                          Arr<int64_t> sinfo, int64_t max_aframes, py::array vsamples, py::array asamples,
                          py::array rinfo, py::array out, Arr<int64_t> out_off, int64_t audio_gap) {
    const int64_t B = es_off.size();
    if (max_aframes <= 0) throw std::invalid_argument("remux_batch: max_aframes must be positive");
    if (audio_gap < 0 || audio_gap % 16 || audio_gap >= (int64_t(1) << 30))
      throw std::invalid_argument("remux_batch: audio_gap must be a non-negative multiple of 16");
    const es::RemuxTables tables{mut_ptr<int32_t>(vsamples, "vsamples"), mut_ptr<int32_t>(asamples, "asamples"),
                                 mut_ptr<int64_t>(rinfo, "rinfo")};
    uint8_t* op = mut_ptr<uint8_t>(out, "out");
    const int64_t* oo = out_off.data();
    const bool sized = out_off.size() == B && vsamples.size() >= table_words(B, max_pes, es::kVsampleWords) &&
                       asamples.size() >= table_words(B, max_aframes, es::kAsampleWords) &&
                       rinfo.size() >= B * es::kRinfoWords;
    const auto region_ok = [&](int64_t b) {
      if (oo[b] < 0 || oo[b] + es::remux_out_bytes(cap.data()[b], max_nal) + audio_gap > out.size())
        throw std::invalid_argument("remux_batch: output region out of bounds");
    };
    each_segment<const int32_t, const int64_t>("remux_batch", es, es_off, cap, info, pes, max_pes, max_nal, nal, au,
                                               aframes, sinfo, sized, region_ok,
                                               [&](const es::Segment& s, const auto& ix, int64_t b) {
      es::remux_segment(s, ix, max_aframes, es::remux_tables_at(tables, s, max_aframes, b), op + oo[b], audio_gap);
    });
  }, py::arg("es"), py::arg("es_off"), py::arg("cap"), py::arg("info"), py::arg("pes"), py::arg("max_pes"),
     py::arg("max_nal"), py::arg("nal"), py::arg("au"), py::arg("aframes"), py::arg("sinfo"), py::arg("max_aframes"),
     py::arg("vsamples"), py::arg("asamples"), py::arg("rinfo"), py::arg("out"), py::arg("out_off"),
     py::arg("audio_gap") = 0);
  m.def("remux_out_bytes", py::vectorize(&es::remux_out_bytes), py::arg("cap"), py::arg("max_nal"));
  m.def("remux_scratch_words", [](int64_t nseg, int64_t max_nal, int64_t max_aframes) {
    return es::remux_scratch(nseg, max_nal, max_aframes).end;
  }, py::arg("nseg"), py::arg("max_nal"), py::arg("max_aframes"));
  m.attr("ES_RINFO_WORDS") = es::kRinfoWords;
  m.attr("ES_VSAMPLE_WORDS") = es::kVsampleWords;
  m.attr("ES_ASAMPLE_WORDS") = es::kAsampleWords;
  m.attr("ES_DEFAULT_MAX_AFRAMES") = es::kDefaultMaxAframes;
  m.attr("ES_REMUX_TILE") = es::kRemuxTile;
  m.attr("ES_OUT_ALIGN") = es::kOutAlign;
  name_dict(m, "ES_RINFO", {{"status", es::kRStatus}, {"video_payload_bytes", es::kVideoPayloadBytes},
                            {"n_vsamples", es::kNumVsamples}, {"audio_box_offset", es::kAudioBoxOffset},
                            {"audio_payload_bytes", es::kAudioPayloadBytes}, {"n_aframes", es::kNumAframes},
                            {"video_base_dts", es::kVideoBaseDts}, {"audio_base_pts", es::kAudioBasePts}});
  name_dict(m, "ES_RSTATUS", {{"truncated", es::kTruncated}, {"aframe_overflow", es::kAframeOverflow},
                              {"bad_timestamps", es::kBadTimestamps},
                              {"unsupported_video", es::kRemuxUnsupportedVideo}});
  name_dict(m, "ES_SAMPLE_FLAGS", {{"sync", es::kSampleSync}, {"non_sync", es::kSampleNonSync}});

  // Batched CPU moof boxes with the device kernel's layout (docs/FRAGMENT.md): remux_batch's three
  // tables, the index's sinfo, one fparams row per segment, and `out` as remux_batch left it, with
  // `headroom` bytes in front of every region and `audio_gap` in front of every audio box.
  //   fparams: int64[B, ES_FPARAM_WORDS]; finfo: int64[B, ES_FINFO_WORDS]
  m.def("fragment_batch", [](Arr<int64_t> rinfo, Arr<int32_t> vsamples, Arr<int32_t> asamples, Arr<int64_t> sinfo,
                             Arr<int64_t> fparams, int64_t max_pes, int64_t max_aframes, int64_t headroom,
                             int64_t audio_gap, py::array out, py::array finfo,
                             std::optional<Arr<int64_t>> mpainfo) {
    const int64_t B = fparams.size() / es::kFparamWords;
    if (max_pes <= 0 || max_aframes <= 0 || max_pes > 0x7fffffff / 16 || max_aframes > 0x7fffffff / 16)
      throw std::invalid_argument("fragment_batch: max_pes and max_aframes must be positive");
    if (headroom < es::frag_headroom(max_pes))
      throw std::invalid_argument("fragment_batch: headroom below frag_headroom(max_pes)");
    if (audio_gap < es::frag_audio_gap(max_aframes) || audio_gap % 16)
      throw std::invalid_argument("fragment_batch: audio_gap below frag_audio_gap(max_aframes) or no multiple of 16");
    if (fparams.size() != B * es::kFparamWords || rinfo.size() < B * es::kRinfoWords ||
        vsamples.size() < table_words(B, max_pes, es::kVsampleWords) ||
        asamples.size() < table_words(B, max_aframes, es::kAsampleWords) || sinfo.size() < B * es::kSinfoWords ||
        finfo.size() < B * es::kFinfoWords || (mpainfo && mpainfo->size() < B * es::kMpainfoWords))
      throw std::invalid_argument("fragment_batch: an argument is too small");
    uint8_t* op = mut_ptr<uint8_t>(out, "out");
    int64_t* fi = mut_ptr<int64_t>(finfo, "finfo");
    const int64_t* fp = fparams.data();
    for (int64_t b = 0; b < B; ++b) {
      const int64_t oo = fp[b * es::kFparamWords + es::kFpOutOff], region = fp[b * es::kFparamWords + es::kFpRegion];
      if (oo < headroom || region < audio_gap + 32 || oo > out.size() || region > out.size() - oo)
        throw std::invalid_argument("fragment_batch: output region out of bounds");
    }
    for (int64_t b = 0; b < B; ++b) {
      const int64_t* row = fp + b * es::kFparamWords;
      es::fragment_segment(rinfo.data() + b * es::kRinfoWords, vsamples.data() + table_words(b, max_pes, es::kVsampleWords),
                           asamples.data() + table_words(b, max_aframes, es::kAsampleWords),
                           sinfo.data()[b * es::kSinfoWords + es::kAudioSampleRate], row, max_pes, max_aframes, audio_gap,
                           op + row[es::kFpOutOff], fi + b * es::kFinfoWords,
                           mpainfo ? mpainfo->data() + b * es::kMpainfoWords : nullptr);
    }
  }, py::arg("rinfo"), py::arg("vsamples"), py::arg("asamples"), py::arg("sinfo"), py::arg("fparams"), py::arg("max_pes"),
     py::arg("max_aframes"), py::arg("headroom"), py::arg("audio_gap"), py::arg("out"), py::arg("finfo"),
     py::arg("mpainfo") = py::none());
  m.def("moof_video_bytes", py::vectorize(&es::moof_video_bytes), py::arg("m"));
  m.def("moof_audio_bytes", py::vectorize(&es::moof_audio_bytes), py::arg("n"));
  m.def("frag_headroom", &es::frag_headroom, py::arg("max_pes"));
  m.def("frag_audio_gap", &es::frag_audio_gap, py::arg("max_aframes"));
  m.def("time_rel", &es::time_rel, py::arg("x"), py::arg("base"), py::arg("ref"));
  m.def("audio_rescale", &es::audio_rescale, py::arg("t90k"), py::arg("rate"));
  m.attr("ES_FINFO_WORDS") = es::kFinfoWords;
  m.attr("ES_FPARAM_WORDS") = es::kFparamWords;
  name_dict(m, "ES_FINFO", {{"status", es::kFStatus}, {"video_moof_bytes", es::kFVideoMoofBytes},
                            {"audio_moof_bytes", es::kFAudioMoofBytes}, {"video_tfdt", es::kFVideoTfdt},
                            {"audio_tfdt", es::kFAudioTfdt}, {"time_base", es::kFTimeBase},
                            {"n_asamples", es::kFNumAsamples}, {"spare", es::kFSpare}});
  name_dict(m, "ES_FSTATUS", {{"time_clamped", es::kTimeClamped}, {"no_rate", es::kNoRate}});
  name_dict(m, "ES_FPARAM", {{"out_off", es::kFpOutOff}, {"region", es::kFpRegion}, {"sequence", es::kFpSequence},
                             {"time_base", es::kFpTimeBase}, {"time_ref", es::kFpTimeRef}, {"anchor", es::kFpAnchor}});

  // Batched CPU codec configuration with the device kernel's layout (docs/INITSEGMENT.md): the inputs of
  // index_batch and its four outputs.
  //   cinfo: int32[B, ES_CINFO_WORDS]; ps: uint8[B, 2, max_ps]
  m.def("config_batch", [](Arr<uint8_t> es, Arr<int64_t> es_off, Arr<int64_t> cap, Arr<int64_t> info, Arr<int64_t> pes,
                           int64_t max_pes, int64_t max_nal, Arr<int32_t> nal, Arr<int32_t> au, Arr<int32_t> aframes,
                           Arr<int64_t> sinfo, int64_t max_ps, py::array cinfo, py::array ps) {
    const int64_t B = es_off.size();
    if (!es::max_ps_ok(max_ps))
      throw std::invalid_argument("config_batch: max_ps must be a positive multiple of 16 up to 1024");
    int32_t* ci = mut_ptr<int32_t>(cinfo, "cinfo");
    uint8_t* pp = mut_ptr<uint8_t>(ps, "ps");
    const bool sized = cinfo.size() >= B * es::kCinfoWords && ps.size() >= es::ps_bytes(B, max_ps);
    each_segment<const int32_t, const int64_t>("config_batch", es, es_off, cap, info, pes, max_pes, max_nal, nal, au,
                                               aframes, sinfo, sized, no_check,
                                               [&](const es::Segment& s, const auto& ix, int64_t b) {
      es::config_segment(s, ix, max_ps, pp + es::ps_bytes(b, max_ps), ci + b * es::kCinfoWords);
    });
  });
  m.attr("ES_CINFO_WORDS") = es::kCinfoWords;
  m.attr("ES_DEFAULT_MAX_PS") = es::kDefaultMaxPs;
  name_dict(m, "ES_CINFO", {{"status", es::kCStatus}, {"sps_nal", es::kCSpsNal}, {"sps_bytes", es::kCSpsBytes},
                            {"sps_rbsp_bytes", es::kCSpsRbspBytes}, {"pps_nal", es::kCPpsNal},
                            {"pps_bytes", es::kCPpsBytes}, {"profile_idc", es::kCProfileIdc},
                            {"profile_compat", es::kCProfileCompat}, {"level_idc", es::kCLevelIdc},
                            {"chroma_format_idc", es::kCChromaFormatIdc}, {"bit_depth_luma", es::kCBitDepthLuma},
                            {"bit_depth_chroma", es::kCBitDepthChroma}, {"width", es::kCWidth},
                            {"height", es::kCHeight}, {"sar_width", es::kCSarWidth}, {"sar_height", es::kCSarHeight},
                            {"aac_object_type", es::kCAacObjectType}, {"aac_rate_index", es::kCAacRateIndex},
                            {"aac_channel_config", es::kCAacChannelConfig}});
  name_dict(m, "ES_CSTATUS", {{"no_sps", es::kNoSps}, {"no_pps", es::kNoPps}, {"ps_overflow", es::kPsOverflow},
                              {"bad_sps", es::kBadSps}, {"unsupported_video", es::kConfigUnsupportedVideo},
                              {"no_audio_config", es::kNoAudioConfig}});

  // Batched CPU HEVC configuration with the device kernel's layout (docs/INITSEGMENT.md): the inputs of
  // config_batch.
  //   hinfo: int32[B, ES_HINFO_WORDS]; hps: uint8[B, 3, max_ps]
  m.def("hevc_config_batch", [](Arr<uint8_t> es, Arr<int64_t> es_off, Arr<int64_t> cap, Arr<int64_t> info,
                                Arr<int64_t> pes, int64_t max_pes, int64_t max_nal, Arr<int32_t> nal, Arr<int32_t> au,
                                Arr<int32_t> aframes, Arr<int64_t> sinfo, int64_t max_ps, py::array hinfo,
                                py::array hps) {
    const int64_t B = es_off.size();
    if (!es::max_ps_ok(max_ps))
      throw std::invalid_argument("hevc_config_batch: max_ps must be a positive multiple of 16 up to 1024");
    int32_t* hi = mut_ptr<int32_t>(hinfo, "hinfo");
    uint8_t* hp = mut_ptr<uint8_t>(hps, "hps");
    const bool sized = hinfo.size() >= B * es::kHinfoWords && hps.size() >= es::hps_bytes(B, max_ps);
    each_segment<const int32_t, const int64_t>("hevc_config_batch", es, es_off, cap, info, pes, max_pes, max_nal, nal,
                                               au, aframes, sinfo, sized, no_check,
                                               [&](const es::Segment& s, const auto& ix, int64_t b) {
      es::hevc_config_segment(s, ix, max_ps, hp + es::hps_bytes(b, max_ps), hi + b * es::kHinfoWords);
    });
  });
  m.attr("ES_HINFO_WORDS") = es::kHinfoWords;
  m.attr("ES_HPS_ROWS") = es::kHpsRows;
  name_dict(m, "ES_HINFO", {{"status", es::kHStatus}, {"vps_nal", es::kHVpsNal}, {"vps_bytes", es::kHVpsBytes},
                            {"sps_nal", es::kHSpsNal}, {"sps_bytes", es::kHSpsBytes},
                            {"sps_rbsp_bytes", es::kHSpsRbspBytes}, {"pps_nal", es::kHPpsNal},
                            {"pps_bytes", es::kHPpsBytes}, {"profile_space", es::kHProfileSpace},
                            {"tier_flag", es::kHTierFlag}, {"profile_idc", es::kHProfileIdc},
                            {"profile_compat", es::kHProfileCompat}, {"constraint_hi", es::kHConstraintHi},
                            {"constraint_lo", es::kHConstraintLo}, {"level_idc", es::kHLevelIdc},
                            {"num_temporal_layers", es::kHNumTemporalLayers},
                            {"temporal_id_nested", es::kHTemporalIdNested},
                            {"chroma_format_idc", es::kHChromaFormatIdc}, {"bit_depth_luma", es::kHBitDepthLuma},
                            {"bit_depth_chroma", es::kHBitDepthChroma}, {"width", es::kHWidth},
                            {"height", es::kHHeight}});
  name_dict(m, "ES_HSTATUS", {{"no_vps", es::kHNoVps}, {"no_sps", es::kHNoSps}, {"no_pps", es::kHNoPps},
                              {"ps_overflow", es::kHPsOverflow}, {"bad_sps", es::kHBadSps},
                              {"not_hevc", es::kHNotHevc}});

  // Batched CPU SAMPLE-AES decryption in place with the device kernel's result (docs/SAMPLEAES.md): the
  // inputs of remux_batch, of which es and the length column of nal are rewritten.
  //   drk: uint32[B, 44] (expand_key_dec); iv: uint8[B, 16]; enable: uint8[B], 0 = the segment is left alone
  //   sainfo: int64[B, ES_SAINFO_WORDS]
  m.def("sample_decrypt_batch", [](py::array es_rw, Arr<int64_t> es_off, Arr<int64_t> cap, Arr<int64_t> info,
                                   Arr<int64_t> pes, int64_t max_pes, int64_t max_nal, py::array nal_rw,
                                   Arr<int32_t> au, Arr<int32_t> aframes, Arr<int64_t> sinfo, Arr<uint32_t> drk,
                                   Arr<uint8_t> iv, Arr<uint8_t> enable, py::array sainfo) {
    const int64_t B = es_off.size();
    uint8_t* ep = mut_ptr<uint8_t>(es_rw, "es");
    int64_t* sa = mut_ptr<int64_t>(sainfo, "sainfo");
    const Arr<uint8_t> es(es_rw);  // the same bytes: es_rw is contiguous uint8
    if (es.data() != ep) throw std::invalid_argument("sample_decrypt_batch: es must be a contiguous uint8 array");
    const bool sized = drk.size() >= B * es::kAesRoundKeyWords && iv.size() >= B * es::kAesBlock &&
                       enable.size() >= B && sainfo.size() >= B * es::kSaWords;
    const int64_t* eo = es_off.data();
    const uint32_t* rk = drk.data();
    const uint8_t *ivp = iv.data(), *en = enable.data();
    each_segment<int32_t, const int64_t>("sample_decrypt_batch", es, es_off, cap, info, pes, max_pes, max_nal, nal_rw,
                                         au, aframes, sinfo, sized, no_check,
                                         [&](const es::Segment& s, const auto& ix, int64_t b) {
      int64_t* row = sa + b * es::kSaWords;
      if (!en[b]) {
        std::fill(row, row + es::kSaWords, 0);
        return;
      }
      es::sample_decrypt_segment(s, ep + eo[b], ix, rk + b * es::kAesRoundKeyWords, ivp + b * es::kAesBlock, row);
    });
  });
  m.attr("ES_SAINFO_WORDS") = es::kSaWords;
  m.attr("ES_SA_ROUND") = es::kSaRound;
  name_dict(m, "ES_SAINFO", {{"status", es::kSaStatus}, {"protected_nals", es::kSaProtectedNals},
                             {"removed_bytes", es::kSaRemovedBytes}, {"video_blocks", es::kSaVideoBlocks},
                             {"audio_frames", es::kSaAudioFrames}, {"audio_blocks", es::kSaAudioBlocks}});
  name_dict(m, "ES_SASTATUS", {{"truncated", es::kSaTruncated}, {"unsupported_video", es::kSaUnsupportedVideo},
                               {"unsupported_audio", es::kSaUnsupportedAudio},
                               {"partial_audio", es::kSaPartialAudio}});

  // Batched CPU caption extraction with the device kernels' layout (docs/CAPTIONS.md): the inputs of
  // config_batch and an enable byte per segment (0: fill values and an all-zero ccinfo row).
  //   ccsamples: int32[B, max_cc, ES_CCROW_WORDS]; ccpts: int64[B, max_cc]; ccbytes: uint8[B, max_cc, ES_CC_SLOT_BYTES]
  //   cc608: uint8[B, max_cc, 2, ES_CC_FIELD_BYTES]; ccinfo: int64[B, ES_CCINFO_WORDS]
  m.def("caption_batch", [](Arr<uint8_t> es, Arr<int64_t> es_off, Arr<int64_t> cap, Arr<int64_t> info,
                            Arr<int64_t> pes, int64_t max_pes, int64_t max_nal, Arr<int32_t> nal, Arr<int32_t> au,
                            Arr<int32_t> aframes, Arr<int64_t> sinfo, Arr<uint8_t> enable, int64_t max_cc,
                            py::array ccsamples, py::array ccpts, py::array ccbytes, py::array cc608,
                            py::array ccinfo) {
    const int64_t B = es_off.size();
    if (!es::max_cc_ok(max_cc)) throw std::invalid_argument("caption_batch: max_cc must be 1 to 2048");
    const es::CcTables t{mut_ptr<int32_t>(ccsamples, "ccsamples"), mut_ptr<int64_t>(ccpts, "ccpts"),
                         mut_ptr<uint8_t>(ccbytes, "ccbytes"), mut_ptr<uint8_t>(cc608, "cc608"),
                         mut_ptr<int64_t>(ccinfo, "ccinfo")};
    const bool sized = enable.size() >= B && ccsamples.size() >= table_words(B, max_cc, es::kCcRowWords) &&
                       ccpts.size() >= B * max_cc && ccbytes.size() >= B * max_cc * es::kCcSlotBytes &&
                       cc608.size() >= B * max_cc * 2 * es::kCcFieldBytes && ccinfo.size() >= B * es::kCcInfoWords;
    const uint8_t* en = enable.data();
    each_segment<const int32_t, const int64_t>("caption_batch", es, es_off, cap, info, pes, max_pes, max_nal, nal, au,
                                               aframes, sinfo, sized, no_check,
                                               [&](const es::Segment& s, const auto& ix, int64_t b) {
      es::caption_segment(s, ix, en[b] != 0, max_cc, es::cc_tables_at(t, max_cc, b));
    });
  });
  m.attr("ES_CCINFO_WORDS") = es::kCcInfoWords;
  m.attr("ES_CCROW_WORDS") = es::kCcRowWords;
  m.attr("ES_CC_NAL_BYTES") = es::kCcNalBytes;
  m.attr("ES_CC_SLOT_BYTES") = es::kCcSlotBytes;
  m.attr("ES_CC_FIELD_BYTES") = es::kCcFieldBytes;
  m.attr("ES_CC_DEFAULT_MAX") = es::kDefaultMaxCc;
  m.attr("ES_CC_MAX_LIMIT") = es::kMaxCcLimit;
  name_dict(m, "ES_CCINFO", {{"status", es::kCiStatus}, {"n_sei", es::kCiNumSei}, {"n_samples", es::kCiNumSamples},
                             {"n_triples", es::kCiNumTriples}, {"field1_pairs", es::kCiField1Pairs},
                             {"field2_pairs", es::kCiField2Pairs}, {"first_pts", es::kCiFirstPts},
                             {"last_pts", es::kCiLastPts}});
  name_dict(m, "ES_CCROW", {{"nal", es::kCrNal}, {"au", es::kCrAu}, {"size", es::kCrSize}, {"cc_count", es::kCrCount},
                            {"order", es::kCrOrder}, {"field1_pairs", es::kCrField1Pairs},
                            {"field2_pairs", es::kCrField2Pairs}, {"flags", es::kCrFlags}});
  name_dict(m, "ES_CCSTATUS", {{"truncated", es::kCcTruncated}, {"unsupported_video", es::kCcUnsupportedVideo},
                               {"cc_overflow", es::kCcOverflow}, {"sei_clipped", es::kCcSeiClipped}});

  // Batched CPU fragmented-MP4 demux with the device kernels' layout (docs/FMP4DEMUX.md): segment b
  // is buf[off[b], off[b] + len[b]), tracks int64[B, MP4_TRACKS, MP4_TRACK_WORDS].
  //   minfo: int64[B, MP4_MINFO_WORDS]; msamples: int32[B, MP4_TRACKS, max_pes, MP4_MSAMPLE_WORDS]
  //   runs: int64[B, max_run, MP4_RUN_WORDS]; emsg: int64[B, max_emsg, MP4_EMSG_WORDS]
  //   info / pes as demux_batch writes them, nal / au / aframes / sinfo as index_batch does
  m.def("mp4_demux_batch", [](Arr<uint8_t> buf, Arr<int64_t> off, Arr<int64_t> len, Arr<int64_t> tracks,
                              int64_t max_pes, int64_t max_nal, int64_t max_moof, int64_t max_run, int64_t max_emsg,
                              py::array minfo, py::array msamples, py::array runs, py::array emsg, py::array info,
                              py::array pes, py::array nal, py::array au, py::array aframes, py::array sinfo) {
    const int64_t B = off.size();
    if (max_pes <= 0 || max_nal <= 0 || !mp4::max_rows_ok(max_moof) || !mp4::max_rows_ok(max_run) ||
        !mp4::max_rows_ok(max_emsg))
      throw std::invalid_argument("mp4_demux_batch: max_pes and max_nal must be positive, max_moof / max_run / "
                                  "max_emsg 1 to 256");
    const mp4::Limits lim{max_pes, max_nal, max_moof, max_run, max_emsg};
    const mp4::Tables t{mut_ptr<int64_t>(minfo, "minfo"), mut_ptr<int32_t>(msamples, "msamples"),
                        mut_ptr<int64_t>(runs, "runs"), mut_ptr<int64_t>(emsg, "emsg"), mut_ptr<int64_t>(info, "info"),
                        mut_ptr<int64_t>(pes, "pes"),
                        {mut_ptr<int32_t>(nal, "nal"), mut_ptr<int32_t>(au, "au"), mut_ptr<int32_t>(aframes, "aframes"),
                         mut_ptr<int64_t>(sinfo, "sinfo")}};
    if (len.size() != B || tracks.size() < B * mp4::kTracks * mp4::kTrackWords || minfo.size() < B * mp4::kMinfoWords ||
        msamples.size() < table_words(B, mp4::kTracks * max_pes, mp4::kMsampleWords) ||
        runs.size() < table_words(B, max_run, mp4::kRunWords) || emsg.size() < table_words(B, max_emsg, mp4::kEmsgWords) ||
        info.size() < B * ts::kInfoWords || pes.size() < ts::pes_words(B, max_pes) ||
        nal.size() < table_words(B, max_nal, es::kNalWords) || au.size() < table_words(B, max_pes, es::kAuWords) ||
        aframes.size() < table_words(B, max_pes, es::kApesWords) || sinfo.size() < B * es::kSinfoWords)
      throw std::invalid_argument("mp4_demux_batch: an argument is too small");
    const int64_t *o = off.data(), *l = len.data();
    int64_t total = 0;
    for (int64_t b = 0; b < B; ++b) {
      if (o[b] < 0 || l[b] < 0 || l[b] >= (int64_t(1) << 31) || o[b] + l[b] > buf.size())
        throw std::invalid_argument("mp4_demux_batch: segment out of bounds");
      total += l[b];
    }
    const uint8_t* base = buf.data();
    const int64_t* tk = tracks.data();
    py::gil_scoped_release nogil;
    parallel_for(B, [&](int64_t b) {
      mp4::demux_segment(base + o[b], l[b], tk + b * mp4::kTracks * mp4::kTrackWords, lim, mp4::tables_at(t, lim, b));
    }, total);
  });
  m.attr("MP4_TRACKS") = mp4::kTracks;
  m.attr("MP4_TRACK_WORDS") = mp4::kTrackWords;
  m.attr("MP4_MINFO_WORDS") = mp4::kMinfoWords;
  m.attr("MP4_MINFO_TRACK0") = mp4::kMTrack0;
  m.attr("MP4_MINFO_TRACK_WORDS") = mp4::kMTrackWords;
  m.attr("MP4_MSAMPLE_WORDS") = mp4::kMsampleWords;
  m.attr("MP4_RUN_WORDS") = mp4::kRunWords;
  m.attr("MP4_EMSG_WORDS") = mp4::kEmsgWords;
  m.attr("MP4_MAX_BOX_ROWS") = mp4::kMaxBoxRows;
  m.attr("MP4_DEFAULT_MAX_MOOF") = mp4::kDefaultMaxMoof;
  m.attr("MP4_DEFAULT_MAX_RUN") = mp4::kDefaultMaxRun;
  m.attr("MP4_DEFAULT_MAX_EMSG") = mp4::kDefaultMaxEmsg;
  name_dict(m, "MP4_TRACK", {{"id", mp4::kTkId}, {"kind", mp4::kTkKind}, {"codec_type", mp4::kTkCodecType},
                             {"nal_length_size", mp4::kTkNalLengthSize}, {"default_duration", mp4::kTkDefDuration},
                             {"default_size", mp4::kTkDefSize}, {"default_flags", mp4::kTkDefFlags}});
  name_dict(m, "MP4_KIND", {{"none", mp4::kKindNone}, {"video", mp4::kKindVideo}, {"audio", mp4::kKindAudio}});
  name_dict(m, "MP4_MINFO", {{"status", mp4::kMStatus}, {"n_moof", mp4::kMNumMoof},
                             {"first_sequence", mp4::kMFirstSequence}, {"n_run", mp4::kMNumRun},
                             {"n_other_traf", mp4::kMNumOtherTraf}, {"n_emsg", mp4::kMNumEmsg}});
  name_dict(m, "MP4_MINFO_TRACK", {{"n_samples", mp4::kMtNumSamples}, {"base_time", mp4::kMtBaseTime},
                                   {"duration", mp4::kMtDuration}, {"min_pts", mp4::kMtMinPts},
                                   {"max_pts", mp4::kMtMaxPts}, {"first_sync", mp4::kMtFirstSync}});
  name_dict(m, "MP4_STATUS", {{"bad_box", mp4::kBadBox}, {"moof_overflow", mp4::kMoofOverflow},
                              {"emsg_overflow", mp4::kEmsgOverflow}, {"run_overflow", mp4::kRunOverflow},
                              {"no_tfdt", mp4::kNoTfdt}, {"sample_out_of_range", mp4::kSampleOutOfRange},
                              {"sample_overflow", mp4::kSampleOverflow}, {"nal_error", mp4::kNalError},
                              {"bad_timestamps", mp4::kBadTimestamps}});
  name_dict(m, "MP4_MSAMPLE", {{"size", mp4::kMsSize}, {"duration", mp4::kMsDuration}, {"cts", mp4::kMsCts},
                               {"flags", mp4::kMsFlags}});
  name_dict(m, "MP4_RUN", {{"track", mp4::kRnTrack}, {"moof", mp4::kRnMoof}, {"first", mp4::kRnFirst},
                           {"count", mp4::kRnCount}, {"entries", mp4::kRnEntries}, {"flags", mp4::kRnFlags},
                           {"traf_run", mp4::kRnTrafRun}, {"default_duration", mp4::kRnDefDuration},
                           {"default_size", mp4::kRnDefSize}, {"default_flags", mp4::kRnDefFlags},
                           {"first_flags", mp4::kRnFirstFlags}, {"start", mp4::kRnStart},
                           {"start_sample", mp4::kRnStartSample}, {"time", mp4::kRnTime},
                           {"time_sample", mp4::kRnTimeSample}});
  name_dict(m, "MP4_EMSG", {{"offset", mp4::kEmOffset}, {"size", mp4::kEmSize}, {"version", mp4::kEmVersion},
                            {"timescale", mp4::kEmTimescale}, {"time", mp4::kEmTime},
                            {"time_is_delta", mp4::kEmTimeIsDelta}, {"duration", mp4::kEmDuration}, {"id", mp4::kEmId},
                            {"data_offset", mp4::kEmDataOffset}, {"data_length", mp4::kEmDataLength},
                            {"is_id3", mp4::kEmIsId3}});

  // Batched CPU packed-audio demux with the device kernel's layout (docs/PACKEDAUDIO.md): segment b
  // is buf[off[b], off[b] + len[b]).
  //   info / pes as demux_batch writes them; nal (one row) / au / aframes / sinfo as index_batch does
  //   painfo: int64[B, ES_PAINFO_WORDS]
  m.def("packed_audio_batch", [](Arr<uint8_t> buf, Arr<int64_t> off, Arr<int64_t> len, int64_t max_pes, py::array info,
                                 py::array pes, py::array nal, py::array au, py::array aframes, py::array sinfo,
                                 py::array painfo) {
    const int64_t B = off.size();
    if (!es::packed_max_pes_ok(max_pes)) throw std::invalid_argument("packed_audio_batch: max_pes must be 1 to 4096");
    const es::PackedTables t{mut_ptr<int64_t>(info, "info"), mut_ptr<int64_t>(pes, "pes"),
                             {mut_ptr<int32_t>(nal, "nal"), mut_ptr<int32_t>(au, "au"),
                              mut_ptr<int32_t>(aframes, "aframes"), mut_ptr<int64_t>(sinfo, "sinfo")},
                             mut_ptr<int64_t>(painfo, "painfo")};
    if (len.size() != B || info.size() < B * ts::kInfoWords || pes.size() < ts::pes_words(B, max_pes) ||
        nal.size() < table_words(B, es::kPackedNalRows, es::kNalWords) ||
        au.size() < table_words(B, max_pes, es::kAuWords) || aframes.size() < table_words(B, max_pes, es::kApesWords) ||
        sinfo.size() < B * es::kSinfoWords || painfo.size() < B * es::kPainfoWords)
      throw std::invalid_argument("packed_audio_batch: an argument is too small");
    const int64_t *o = off.data(), *l = len.data();
    int64_t total = 0;
    for (int64_t b = 0; b < B; ++b) {
      if (o[b] < 0 || l[b] < 0 || l[b] >= (int64_t(1) << 31) || o[b] + l[b] > buf.size())
        throw std::invalid_argument("packed_audio_batch: segment out of bounds");
      total += l[b];
    }
    const uint8_t* base = buf.data();
    py::gil_scoped_release nogil;
    parallel_for(B, [&](int64_t b) {
      es::packed_segment(base + o[b], l[b], max_pes, es::packed_tables_at(t, max_pes, b));
    }, total);
  });
  // Batched CPU MPEG audio behind remux_batch with the device kernels' layout (docs/MPEGAUDIO.md):
  // the demuxed batch, per segment the bytes of its output region (the audio gap included), and the
  // remux's asamples, rinfo and out, which are rewritten for a segment with an MPEG audio config.
  //   mframes: int32[B, max_pes, ES_APES_WORDS]; mpainfo: int64[B, ES_MPAINFO_WORDS]
  m.def("mpeg_audio_batch", [](Arr<uint8_t> es, Arr<int64_t> es_off, Arr<int64_t> cap, Arr<int64_t> info, Arr<int64_t> pes,
                               int64_t max_pes, Arr<int64_t> region, int64_t max_aframes, py::array mframes,
                               py::array mpainfo, py::array asamples, py::array rinfo, py::array out,
                               Arr<int64_t> out_off) {
    const int64_t B = es_off.size();
    if (max_pes <= 0 || max_aframes <= 0) throw std::invalid_argument("mpeg_audio_batch: max_pes and max_aframes must be positive");
    if (cap.size() != B || region.size() != B || out_off.size() != B || info.size() < B * ts::kInfoWords ||
        pes.size() < ts::pes_words(B, max_pes) || mframes.size() < table_words(B, max_pes, es::kApesWords) ||
        mpainfo.size() < B * es::kMpainfoWords || asamples.size() < table_words(B, max_aframes, es::kAsampleWords) ||
        rinfo.size() < B * es::kRinfoWords)
      throw std::invalid_argument("mpeg_audio_batch: an argument is too small");
    const es::MpaTables t{mut_ptr<int32_t>(mframes, "mframes"), mut_ptr<int64_t>(mpainfo, "mpainfo"),
                          mut_ptr<int32_t>(asamples, "asamples"), mut_ptr<int64_t>(rinfo, "rinfo")};
    uint8_t* op = mut_ptr<uint8_t>(out, "out");
    const int64_t *eo = es_off.data(), *cp = cap.data(), *rg = region.data(), *oo = out_off.data();
    for (int64_t b = 0; b < B; ++b) {
      if (eo[b] < 0 || cp[b] < 0 || eo[b] + cp[b] > es.size()) throw std::invalid_argument("mpeg_audio_batch: ES out of bounds");
      if (oo[b] < 0 || rg[b] < 16 || oo[b] > out.size() || rg[b] > out.size() - oo[b])
        throw std::invalid_argument("mpeg_audio_batch: output region out of bounds");
    }
    const uint8_t* ep = es.data();
    const int64_t *ip = info.data(), *pp = pes.data();
    py::gil_scoped_release nogil;
    for (int64_t b = 0; b < B; ++b) {
      const es::Segment s = es::segment_at(ep, eo, cp, ip, pp, max_pes, 0, b);
      es::mpeg_audio_segment(s, rg[b], max_aframes,
                             {t.mframes + table_words(b, max_pes, es::kApesWords), t.mpainfo + b * es::kMpainfoWords,
                              t.asamples + table_words(b, max_aframes, es::kAsampleWords), t.rinfo + b * es::kRinfoWords},
                             op + oo[b]);
    }
  });
  m.def("mpa_frame", [](Arr<uint8_t> bytes, int64_t q, int64_t end) {
    if (q < 0 || end > bytes.size()) throw std::invalid_argument("mpa_frame: range outside the bytes");
    const es::MpaFrame f = es::mpa_frame_at(bytes.data(), q, end);
    return py::make_tuple(f.len, f.counts, f.key, f.samples, f.rate, f.channels, f.version, f.layer, f.bitrate);
  }, py::arg("bytes"), py::arg("q"), py::arg("end"));
  m.def("mpa_scratch_words", [](int64_t nseg, int64_t max_pes) { return es::mpa_scratch(nseg, max_pes).end; },
        py::arg("nseg"), py::arg("max_pes"));
  m.attr("ES_MPAINFO_WORDS") = es::kMpainfoWords;
  name_dict(m, "ES_MPAINFO", {{"status", es::kMpStatus}, {"n_frames", es::kMpNumFrames}, {"sample_rate", es::kMpSampleRate},
                              {"channels", es::kMpChannels}, {"version", es::kMpVersion}, {"layer", es::kMpLayer},
                              {"frame_samples", es::kMpFrameSamples}, {"bitrate", es::kMpBitrate}});
  name_dict(m, "ES_MPASTATUS", {{"not_mpeg_audio", es::kMpaNotMpegAudio}, {"no_audio_config", es::kMpaNoAudioConfig},
                                {"mpa_error", es::kMpaError}, {"format_change", es::kMpaFormatChange},
                                {"aframe_overflow", es::kMpaAframeOverflow}});
  // Batched CPU AC-3 / E-AC-3 audio behind remux_batch (and mpeg_audio_batch) with the device
  // kernels' layout (docs/AC3AUDIO.md): mpeg_audio_batch's arguments, with ac3info and a new row in
  // mpainfo's layout per segment; mpa_in is the MPEG audio op's mpainfo (only read) or None.
  //   dframes: int32[B, max_pes, ES_APES_WORDS]; ac3info: int64[B, ES_AC3INFO_WORDS]; mpainfo: int64[B, ES_MPAINFO_WORDS]
  m.def("ac3_audio_batch", [](Arr<uint8_t> es, Arr<int64_t> es_off, Arr<int64_t> cap, Arr<int64_t> info, Arr<int64_t> pes,
                              int64_t max_pes, Arr<int64_t> region, int64_t max_aframes, py::array dframes,
                              py::array ac3info, py::array mpainfo, py::array asamples, py::array rinfo, py::array out,
                              Arr<int64_t> out_off, std::optional<Arr<int64_t>> mpa_in) {
    const int64_t B = es_off.size();
    if (max_pes <= 0 || max_aframes <= 0) throw std::invalid_argument("ac3_audio_batch: max_pes and max_aframes must be positive");
    if (cap.size() != B || region.size() != B || out_off.size() != B || info.size() < B * ts::kInfoWords ||
        pes.size() < ts::pes_words(B, max_pes) || dframes.size() < table_words(B, max_pes, es::kApesWords) ||
        ac3info.size() < B * es::kAc3infoWords || mpainfo.size() < B * es::kMpainfoWords ||
        asamples.size() < table_words(B, max_aframes, es::kAsampleWords) || rinfo.size() < B * es::kRinfoWords ||
        (mpa_in && mpa_in->size() < B * es::kMpainfoWords))
      throw std::invalid_argument("ac3_audio_batch: an argument is too small");
    const es::Ac3Tables t{mut_ptr<int32_t>(dframes, "dframes"), mut_ptr<int64_t>(ac3info, "ac3info"),
                          mut_ptr<int64_t>(mpainfo, "mpainfo"), mpa_in ? mpa_in->data() : nullptr,
                          mut_ptr<int32_t>(asamples, "asamples"), mut_ptr<int64_t>(rinfo, "rinfo")};
    uint8_t* op = mut_ptr<uint8_t>(out, "out");
    const int64_t *eo = es_off.data(), *cp = cap.data(), *rg = region.data(), *oo = out_off.data();
    for (int64_t b = 0; b < B; ++b) {
      if (eo[b] < 0 || cp[b] < 0 || eo[b] + cp[b] > es.size()) throw std::invalid_argument("ac3_audio_batch: ES out of bounds");
      if (oo[b] < 0 || rg[b] < 16 || oo[b] > out.size() || rg[b] > out.size() - oo[b])
        throw std::invalid_argument("ac3_audio_batch: output region out of bounds");
    }
    const uint8_t* ep = es.data();
    const int64_t *ip = info.data(), *pp = pes.data();
    py::gil_scoped_release nogil;
    for (int64_t b = 0; b < B; ++b) {
      const es::Segment s = es::segment_at(ep, eo, cp, ip, pp, max_pes, 0, b);
      es::ac3_audio_segment(s, rg[b], max_aframes,
                            {t.dframes + table_words(b, max_pes, es::kApesWords), t.ac3info + b * es::kAc3infoWords,
                             t.mpainfo + b * es::kMpainfoWords, t.mpa_in ? t.mpa_in + b * es::kMpainfoWords : nullptr,
                             t.asamples + table_words(b, max_aframes, es::kAsampleWords), t.rinfo + b * es::kRinfoWords},
                            op + oo[b]);
    }
  }, py::arg("es"), py::arg("es_off"), py::arg("cap"), py::arg("info"), py::arg("pes"), py::arg("max_pes"),
     py::arg("region"), py::arg("max_aframes"), py::arg("dframes"), py::arg("ac3info"), py::arg("mpainfo"),
     py::arg("asamples"), py::arg("rinfo"), py::arg("out"), py::arg("out_off"), py::arg("mpa_in") = py::none());
  m.def("ac3_frame", [](Arr<uint8_t> bytes, int64_t q, int64_t end) {
    if (q < 0 || end > bytes.size()) throw std::invalid_argument("ac3_frame: range outside the bytes");
    const es::Ac3Frame f = es::ac3_frame_at(bytes.data(), q, end);
    return py::make_tuple(f.len, f.counts, f.key, f.layout_ok, f.kind, f.rate, f.channels, f.bsid, f.bitrate, f.fscod,
                          f.bsmod, f.acmod, f.lfeon, f.bit_rate_code, f.data_rate);
  }, py::arg("bytes"), py::arg("q"), py::arg("end"));
  m.attr("ES_AC3INFO_WORDS") = es::kAc3infoWords;
  m.attr("ES_AC3_FRAME_SAMPLES") = es::kAc3FrameSamples;
  name_dict(m, "ES_AC3INFO", {{"status", es::kAcStatus}, {"n_frames", es::kAcNumFrames}, {"sample_rate", es::kAcSampleRate},
                              {"channels", es::kAcChannels}, {"kind", es::kAcKind}, {"bsid", es::kAcBsid},
                              {"frame_samples", es::kAcFrameSamples}, {"bitrate", es::kAcBitrate}, {"fscod", es::kAcFscod},
                              {"bsmod", es::kAcBsmod}, {"acmod", es::kAcAcmod}, {"lfeon", es::kAcLfeon},
                              {"bit_rate_code", es::kAcBitRateCode}, {"data_rate", es::kAcDataRate},
                              {"first_frame_bytes", es::kAcFirstFrameBytes}});
  name_dict(m, "ES_AC3STATUS", {{"not_dolby_audio", es::kAc3NotDolbyAudio}, {"no_audio_config", es::kAc3NoAudioConfig},
                                {"ac3_error", es::kAc3Error}, {"format_change", es::kAc3FormatChange},
                                {"aframe_overflow", es::kAc3AframeOverflow},
                                {"unsupported_layout", es::kAc3UnsupportedLayout}});
  m.attr("ES_PAINFO_WORDS") = es::kPainfoWords;
  m.attr("ES_PACKED_FRAMES_PER_PES") = es::kPackedFramesPerPes;
  m.attr("ES_PACKED_MAX_TAGS") = es::kPackedMaxTags;
  m.attr("ES_PACKED_MAX_ID3_FRAMES") = es::kPackedMaxId3Frames;
  m.attr("ES_PACKED_NAL_ROWS") = es::kPackedNalRows;
  m.attr("ES_PACKED_TILE") = es::kPackedTile;
  m.attr("ES_PACKED_MAX_PES_LIMIT") = es::kPackedMaxPesLimit;
  m.attr("ES_PACKED_FATAL") = static_cast<int64_t>(es::kPaFatalMask);
  name_dict(m, "ES_PAINFO", {{"status", es::kPaStatus}, {"id3_bytes", es::kPaId3Bytes}, {"n_tags", es::kPaNumTags},
                             {"timestamp", es::kPaTimestamp}, {"n_frames", es::kPaNumFrames},
                             {"stop_offset", es::kPaStopOffset}, {"sample_rate", es::kPaSampleRate},
                             {"channels", es::kPaChannels}});
  name_dict(m, "ES_PASTATUS", {{"no_timestamp", es::kPaNoTimestamp}, {"bad_id3", es::kPaBadId3},
                               {"no_frame", es::kPaNoFrame}, {"trailing_bytes", es::kPaTrailingBytes},
                               {"pes_overflow", es::kPaPesOverflow}, {"bad_rate", es::kPaBadRate}});

  // Batched CPU cbcs decryption with the device kernels' result (docs/CBCS.md): segment b is
  // src[src_off[b], + len[b]), only read, and dst[dst_off[b], + len[b]) already holds its copy; a
  // segment with enable 0 is left alone (all-zero cinfo row, -1 ranges).
  //   minfo / msamples / runs / info / pes: as mp4_demux_batch wrote them
  //   prot: int64[B, MP4_TRACKS, CBCS_PROT_WORDS]; const_iv: uint8[B, MP4_TRACKS, 16]; iv: uint8[B, 16]
  //   drk: uint32[B, 44] (expand_key_dec); ranges: int32[B, max_range, CBCS_RANGE_WORDS]; cinfo: int64[B, CBCS_CINFO_WORDS]
  // cbcs and cenc share the checks and the batch loop: op names the call in messages, the row
  // widths are the scheme's and segment is mp4::cbcs_segment or mp4::cenc_segment
  static const auto protected_batch = [](const char* op, int range_words, int info_words, auto segment,
                                         Arr<uint8_t> src, Arr<int64_t> src_off, Arr<int64_t> len, py::array dst_rw,
                                         Arr<int64_t> dst_off, Arr<int64_t> minfo, Arr<int32_t> msamples,
                                         Arr<int64_t> runs, Arr<int64_t> info, Arr<int64_t> pes, int64_t max_pes,
                                         int64_t max_run, Arr<int64_t> prot, Arr<uint8_t> const_iv, Arr<uint8_t> iv,
                                         Arr<uint32_t> drk, Arr<uint8_t> enable, int64_t max_range, py::array ranges,
                                         py::array cinfo) {
    const std::string name(op);
    const int64_t B = src_off.size();
    if (max_pes <= 0 || !mp4::max_rows_ok(max_run) || !mp4::max_range_ok(max_range))
      throw std::invalid_argument(name + ": max_pes must be positive, max_run 1 to 256, max_range 1 to 65536");
    uint8_t* dp = mut_ptr<uint8_t>(dst_rw, "dst");
    int32_t* rg = mut_ptr<int32_t>(ranges, "ranges");
    int64_t* ci = mut_ptr<int64_t>(cinfo, "cinfo");
    if (len.size() != B || dst_off.size() != B || minfo.size() < B * mp4::kMinfoWords ||
        msamples.size() < table_words(B, mp4::kTracks * max_pes, mp4::kMsampleWords) ||
        runs.size() < table_words(B, max_run, mp4::kRunWords) || info.size() < B * ts::kInfoWords ||
        pes.size() < ts::pes_words(B, max_pes) || prot.size() < B * mp4::kTracks * mp4::kProtWords ||
        const_iv.size() < B * mp4::kTracks * es::kAesBlock || iv.size() < B * es::kAesBlock ||
        drk.size() < B * es::kAesRoundKeyWords || enable.size() < B ||
        ranges.size() < table_words(B, max_range, range_words) || cinfo.size() < B * info_words)
      throw std::invalid_argument(name + ": an argument is too small");
    const int64_t *so = src_off.data(), *l = len.data(), *dof = dst_off.data();
    const uint8_t* en = enable.data();
    int64_t total = 0;
    for (int64_t b = 0; b < B; ++b) {
      if (!en[b]) continue;
      if (so[b] < 0 || l[b] < 0 || l[b] >= (int64_t(1) << 31) || so[b] + l[b] > src.size() || dof[b] < 0 ||
          dof[b] + l[b] > dst_rw.size())
        throw std::invalid_argument(name + ": segment out of bounds");
      total += l[b];
    }
    const uint8_t* sp = src.data();
    if (sp == dp) throw std::invalid_argument(name + ": cannot run in place");
    const int64_t *mi = minfo.data(), *rn = runs.data(), *in = info.data(), *pe = pes.data(), *pr = prot.data();
    const int32_t* ms = msamples.data();
    const uint8_t *civ = const_iv.data(), *ivp = iv.data();
    const uint32_t* rk = drk.data();
    py::gil_scoped_release nogil;
    parallel_for(B, [&](int64_t b) {
      int32_t* rows = rg + table_words(b, max_range, range_words);
      int64_t* row = ci + b * info_words;
      if (!en[b]) {
        std::fill(rows, rows + table_words(1, max_range, range_words), -1);
        std::fill(row, row + info_words, int64_t(0));
        return;
      }
      const mp4::CbcsDemux md{mi + b * mp4::kMinfoWords, rn + table_words(b, max_run, mp4::kRunWords),
                              in + b * ts::kInfoWords, pe + ts::pes_words(b, max_pes),
                              ms + table_words(b, mp4::kTracks * max_pes, mp4::kMsampleWords), max_pes, max_run};
      segment(sp + so[b], l[b], md, pr + b * mp4::kTracks * mp4::kProtWords, civ + b * mp4::kTracks * es::kAesBlock,
              ivp + b * es::kAesBlock, rk + b * es::kAesRoundKeyWords, max_range, dp + dof[b], rows, row);
    }, total);
  };
  m.def("cbcs_decrypt_batch", [](Arr<uint8_t> src, Arr<int64_t> src_off, Arr<int64_t> len, py::array dst_rw,
                                 Arr<int64_t> dst_off, Arr<int64_t> minfo, Arr<int32_t> msamples, Arr<int64_t> runs,
                                 Arr<int64_t> info, Arr<int64_t> pes, int64_t max_pes, int64_t max_run,
                                 Arr<int64_t> prot, Arr<uint8_t> const_iv, Arr<uint8_t> iv, Arr<uint32_t> drk,
                                 Arr<uint8_t> enable, int64_t max_range, py::array ranges, py::array cinfo) {
    protected_batch("cbcs_decrypt_batch", mp4::kRangeWords, mp4::kCbInfoWords, &mp4::cbcs_segment, src, src_off, len,
                    dst_rw, dst_off, minfo, msamples, runs, info, pes, max_pes, max_run, prot, const_iv, iv, drk, enable,
                    max_range, ranges, cinfo);
  });
  m.attr("CBCS_PROT_WORDS") = mp4::kProtWords;
  m.attr("CBCS_CINFO_WORDS") = mp4::kCbInfoWords;
  m.attr("CBCS_RANGE_WORDS") = mp4::kRangeWords;
  m.attr("CBCS_AUX_WORDS") = mp4::kAuxWords;
  m.attr("CBCS_TRACK_SHIFT") = mp4::kRgTrackShift;
  m.attr("CBCS_MAX_RANGE_LIMIT") = mp4::kMaxRangeLimit;
  m.attr("CBCS_DEFAULT_MAX_RANGE") = mp4::kDefaultMaxRange;
  name_dict(m, "CBCS_PROT", {{"protected", mp4::kPrProtected}, {"crypt", mp4::kPrCrypt}, {"skip", mp4::kPrSkip},
                             {"per_sample_iv_size", mp4::kPrIvSize}, {"constant_iv_size", mp4::kPrConstIvSize}});
  name_dict(m, "CBCS_CINFO", {{"status", mp4::kCbStatus}, {"n_ranges", mp4::kCbNumRanges},
                              {"video_samples", mp4::kCbVideoSamples}, {"audio_samples", mp4::kCbAudioSamples},
                              {"video_blocks", mp4::kCbVideoBlocks}, {"audio_blocks", mp4::kCbAudioBlocks},
                              {"n_senc", mp4::kCbNumSenc}});
  name_dict(m, "CBCS_STATUS", {{"range_overflow", mp4::kCbRangeOverflow}, {"no_senc", mp4::kCbNoSenc},
                               {"bad_senc", mp4::kCbBadSenc}, {"demux_damaged", mp4::kCbDemuxDamaged},
                               {"overlap", mp4::kCbOverlap}});
  name_dict(m, "CBCS_RANGE", {{"offset", mp4::kRgOffset}, {"length", mp4::kRgLength}, {"sample", mp4::kRgSample},
                              {"rank", mp4::kRgRank}});

  // Batched CPU cenc (AES-CTR) decryption with the device kernels' result (docs/CENC.md): the
  // arguments of cbcs_decrypt_batch, but
  //   erk: uint32[B, 44] (expand_key_enc); ranges: int32[B, max_range, CENC_RANGE_WORDS]; cinfo: int64[B, CENC_CINFO_WORDS]
  m.def("cenc_decrypt_batch", [](Arr<uint8_t> src, Arr<int64_t> src_off, Arr<int64_t> len, py::array dst_rw,
                                 Arr<int64_t> dst_off, Arr<int64_t> minfo, Arr<int32_t> msamples, Arr<int64_t> runs,
                                 Arr<int64_t> info, Arr<int64_t> pes, int64_t max_pes, int64_t max_run,
                                 Arr<int64_t> prot, Arr<uint8_t> const_iv, Arr<uint8_t> iv, Arr<uint32_t> erk,
                                 Arr<uint8_t> enable, int64_t max_range, py::array ranges, py::array cinfo) {
    protected_batch("cenc_decrypt_batch", mp4::kCnRangeWords, mp4::kCnInfoWords, &mp4::cenc_segment, src, src_off, len,
                    dst_rw, dst_off, minfo, msamples, runs, info, pes, max_pes, max_run, prot, const_iv, iv, erk, enable,
                    max_range, ranges, cinfo);
  });
  m.attr("CENC_CINFO_WORDS") = mp4::kCnInfoWords;
  m.attr("CENC_RANGE_WORDS") = mp4::kCnRangeWords;
  m.attr("CENC_TILE_UNITS") = mp4::kCnTileUnits;
  name_dict(m, "CENC_CINFO", {{"status", mp4::kCnStatus}, {"n_ranges", mp4::kCnNumRanges},
                              {"video_samples", mp4::kCnVideoSamples}, {"audio_samples", mp4::kCnAudioSamples},
                              {"video_bytes", mp4::kCnVideoBytes}, {"audio_bytes", mp4::kCnAudioBytes},
                              {"n_senc", mp4::kCnNumSenc}, {"n_units", mp4::kCnNumUnits}});
  name_dict(m, "CENC_RANGE", {{"offset", mp4::kCnOffset}, {"length", mp4::kCnLength}, {"sample", mp4::kCnSample},
                              {"rank", mp4::kCnRank}, {"stream_pos", mp4::kCnStreamPos},
                              {"iv_offset", mp4::kCnIvOffset}});

  // ------------------------------------------------------------------ store
  m.def("key_digest", [](Arr<int64_t> keys) {
    // int64[n, 4] segment keys -> uint32[n]: the digest a keyed CRC is bound with
    if (keys.size() % 4) throw std::invalid_argument("key_digest: keys must be int64[n, 4]");
    const int64_t n = keys.size() / 4;
    Arr<uint32_t> out(n);
    for (int64_t i = 0; i < n; ++i) out.mutable_data()[i] = key_digest(key_from(keys.data() + 4 * i));
    return out;
  });
  py::class_<SegmentStore>(m, "SegmentStore")
      .def(py::init<int64_t, int64_t>(), py::arg("capacity"), py::arg("align") = 256)
      .def_property_readonly("capacity", &SegmentStore::capacity)
      .def_property_readonly("used_bytes", &SegmentStore::used_bytes)
      .def_property_readonly("num_entries", &SegmentStore::num_entries)
      .def_property_readonly("evictions", &SegmentStore::evictions)
      .def_property_readonly("max_entries", &SegmentStore::max_entries)
      .def("lookup", [](const SegmentStore& s, Arr<int64_t> keys, bool include_pending) {
        const int64_t n = keys.size() / 4;
        Arr<int64_t> out(n);
        const int64_t* k = keys.data();
        int64_t* o = out.mutable_data();
        for (int64_t i = 0; i < n; ++i) o[i] = s.lookup(key_from(k + 4 * i), include_pending);
        return out;
      }, py::arg("keys"), py::arg("include_pending") = false)
      .def("lookup1", [](const SegmentStore& s, uint32_t swarm, uint32_t level, uint32_t url_id, uint32_t sn) {
        return s.lookup(SegKey{swarm, level, url_id, sn}, false);
      })
      .def("entries", [](const SegmentStore& s, Arr<int64_t> ids) {
        // -> int64[n, 4]: offset, length, state, pins
        const int64_t n = ids.size();
        Arr<int64_t> out({n, int64_t(4)});
        int64_t* o = out.mutable_data();
        for (int64_t i = 0; i < n; ++i) {
          int64_t id = ids.data()[i];
          if (id < 0 || id >= s.max_entries()) throw std::out_of_range("bad entry id");
          const Entry& e = s.entry(id);
          o[4 * i] = e.offset; o[4 * i + 1] = e.length; o[4 * i + 2] = e.state; o[4 * i + 3] = e.pins;
        }
        return out;
      })
      .def("reserve_run", [](SegmentStore& s, Arr<int64_t> keys, Arr<int64_t> lens, int64_t tick) -> py::object {
        const int64_t n = lens.size();
        if (keys.size() != 4 * n) throw std::invalid_argument("keys must be int64[n,4]");
        std::vector<SegKey> k(n);
        for (int64_t i = 0; i < n; ++i) k[i] = key_from(keys.data() + 4 * i);
        Arr<int64_t> ids(n), offs(n);
        int64_t base = s.reserve_run(k.data(), lens.data(), n, tick, ids.mutable_data(), offs.mutable_data());
        if (base < 0) return py::none();
        return py::make_tuple(base, ids, offs);
      })
      .def("p2p_layout", [](SegmentStore& s, Arr<int64_t> send_rows, Arr<int64_t> send_eids, Arr<int64_t> recv_rows,
                            int64_t tick) {
        // One round's P2P buffers (node.py:_p2p_phase), in one call.  Plan rows (sorted by
        // (src, dst, key)): [key x4, len, src, dst, want_id, seeded].
        //  sends, per destination run: (dst, row_a, row_b, mode, offset, total) -- mode 0:
        //    the run's entries lie back to back in the arena (aligned), send arena[offset,
        //    offset + total) as is; mode 1: gather into a staging buffer of `total` bytes,
        //    copies listed in `gathers` (run, arena offset, buffer offset, length).
        //  recvs, per source run: (src, row_a, row_b, base, total) -- one contiguous ring
        //    reservation, entries pinned; rid / roff: entry id / offset per recv row.
        const int64_t ns = send_eids.size();
        const int64_t nr = recv_rows.ndim() == 2 ? recv_rows.shape(0) : 0;
        if (ns && (send_rows.ndim() != 2 || send_rows.shape(0) != ns || send_rows.shape(1) < 9))
          throw std::invalid_argument("send_rows must be int64[n, >=9] aligned with send_eids");
        if (nr && recv_rows.shape(1) < 9) throw std::invalid_argument("recv_rows must be int64[n, >=9]");
        const int64_t sc = ns ? send_rows.shape(1) : 9, rc = nr ? recv_rows.shape(1) : 9;
        const int64_t* sr = send_rows.data();
        const int64_t* se = send_eids.data();
        const int64_t* rr = recv_rows.data();
        std::vector<int64_t> srun, gath;
        for (int64_t a = 0; a < ns;) {
          const int64_t dst = sr[a * sc + 6];
          int64_t b = a + 1;
          while (b < ns && sr[b * sc + 6] == dst) ++b;
          bool contiguous = true;
          int64_t total = 0;
          for (int64_t i = a; i < b && contiguous; ++i) {
            const int64_t id = se[i];
            if (id < 0 || id >= s.max_entries()) { contiguous = false; break; }
            const Entry& e = s.entry(id);
            if (e.length != sr[i * sc + 4]) contiguous = false;
            if (i > a) {
              const Entry& p = s.entry(se[i - 1]);
              if (e.offset != p.offset + s.aligned(p.length)) contiguous = false;
            }
          }
          if (contiguous) {
            const Entry& f = s.entry(se[a]);
            const Entry& l = s.entry(se[b - 1]);
            total = l.offset + l.length - f.offset;
            srun.insert(srun.end(), {dst, a, b, 0, f.offset, total});
          } else {
            const int64_t run = static_cast<int64_t>(srun.size() / 6);
            int64_t pos = 0;
            for (int64_t i = a; i < b; ++i) {
              const int64_t len = sr[i * sc + 4];
              const int64_t id = se[i];
              if (id >= 0 && id < s.max_entries()) {
                const Entry& e = s.entry(id);
                gath.insert(gath.end(), {run, e.offset, pos, std::min(e.length, len)});
              }
              total = pos + len;
              pos += s.aligned(len);
            }
            srun.insert(srun.end(), {dst, a, b, 1, -1, total});
          }
          a = b;
        }
        std::vector<int64_t> rrun;
        Arr<int64_t> rid(nr), roff(nr);
        for (int64_t a = 0; a < nr;) {
          const int64_t src = rr[a * rc + 5];
          int64_t b = a + 1;
          while (b < nr && rr[b * rc + 5] == src) ++b;
          const int64_t n = b - a;
          std::vector<SegKey> keys(n);
          std::vector<int64_t> lens(n);
          for (int64_t i = 0; i < n; ++i) {
            keys[i] = key_from(rr + (a + i) * rc);
            lens[i] = rr[(a + i) * rc + 4];
          }
          const int64_t base = s.reserve_run(keys.data(), lens.data(), n, tick, rid.mutable_data() + a,
                                             roff.mutable_data() + a);
          if (base < 0) throw std::runtime_error("segment cache cannot make room for peer data");
          for (int64_t i = a; i < b; ++i) s.pin(rid.data()[i]);
          const int64_t total = roff.data()[b - 1] + lens[n - 1] - roff.data()[a];
          rrun.insert(rrun.end(), {src, a, b, roff.data()[a], total});
          a = b;
        }
        auto as2d = [](const std::vector<int64_t>& v, int64_t cols) {
          const int64_t rows = static_cast<int64_t>(v.size()) / cols;
          Arr<int64_t> out({rows, cols});
          if (rows) std::memcpy(out.mutable_data(), v.data(), v.size() * sizeof(int64_t));
          return out;
        };
        return py::make_tuple(as2d(srun, 6), as2d(gath, 4), as2d(rrun, 5), rid, roff);
      })
      .def("fits", &SegmentStore::fits)
      // ---- replicated-state audit (agent/audit.py)
      .def("audit", [](const SegmentStore& s) {
        std::vector<std::string> e;
        s.audit(&e);
        return e;
      })
      .def_property_readonly("unpin_underflows", &SegmentStore::unpin_underflows)
      .def("region_start", &SegmentStore::region_start)
      .def("pin_table", [](const SegmentStore& s) {
        // -> (ids int64[n], pins int64[n]) of live entries holding pins
        std::vector<int64_t> ids, pins;
        for (int64_t i = 0; i < s.max_entries(); ++i) {
          const Entry& e = s.entry(i);
          if (e.state != kFree && e.pins != 0) {
            ids.push_back(i);
            pins.push_back(e.pins);
          }
        }
        Arr<int64_t> a(static_cast<py::ssize_t>(ids.size())), b(static_cast<py::ssize_t>(pins.size()));
        if (!ids.empty()) {
          std::memcpy(a.mutable_data(), ids.data(), ids.size() * sizeof(int64_t));
          std::memcpy(b.mutable_data(), pins.data(), pins.size() * sizeof(int64_t));
        }
        return py::make_tuple(a, b);
      })
      .def("live_entries", [](const SegmentStore& s) {
        // -> int64[n, 9]: id, key x4, offset, alloc bytes, state, indexed (the index names it)
        std::vector<int64_t> rows;
        for (int64_t i = 0; i < s.max_entries(); ++i) {
          const Entry& e = s.entry(i);
          if (e.state == kFree) continue;
          const int64_t ix = s.lookup(e.key, true);
          rows.insert(rows.end(), {i, int64_t(e.key.swarm), int64_t(e.key.level), int64_t(e.key.url_id),
                                   int64_t(e.key.sn), e.offset, e.alloc_bytes, int64_t(e.state), ix == i ? 1 : 0});
        }
        const int64_t n = static_cast<int64_t>(rows.size() / 9);
        Arr<int64_t> out({n, int64_t(9)});
        if (n) std::memcpy(out.mutable_data(), rows.data(), rows.size() * sizeof(int64_t));
        return out;
      })
      .def("peek_delta", [](const SegmentStore& s) {
        // -> (added int64[n,4], removed int64[m,4]) not taken yet
        std::vector<SegKey> add, rm;
        s.peek_delta(&add, &rm);
        auto keys = [](const std::vector<SegKey>& v) {
          Arr<int64_t> a({int64_t(v.size()), int64_t(4)});
          int64_t* p = a.mutable_data();
          for (size_t i = 0; i < v.size(); ++i) {
            p[4 * i] = v[i].swarm; p[4 * i + 1] = v[i].level; p[4 * i + 2] = v[i].url_id; p[4 * i + 3] = v[i].sn;
          }
          return a;
        };
        return py::make_tuple(keys(add), keys(rm));
      })
      .def("wrap_for", &SegmentStore::wrap_for)
      .def("retire_region", &SegmentStore::retire_region)
      .def("resident", [](const SegmentStore& s) {
        // -> (ids int64[n], keys int64[n,4]) of resident entries, oldest first
        std::vector<int64_t> ids;
        s.resident_ids(&ids);
        const int64_t n = static_cast<int64_t>(ids.size());
        Arr<int64_t> id_arr(n), keys({n, int64_t(4)});
        int64_t* k = keys.mutable_data();
        for (int64_t i = 0; i < n; ++i) {
          id_arr.mutable_data()[i] = ids[i];
          const SegKey& key = s.entry(ids[i]).key;
          k[4 * i] = key.swarm; k[4 * i + 1] = key.level; k[4 * i + 2] = key.url_id; k[4 * i + 3] = key.sn;
        }
        return py::make_tuple(id_arr, keys);
      })
      .def("aligned", &SegmentStore::aligned)
      .def("commit", [](SegmentStore& s, Arr<int64_t> ids) {
        for (int64_t i = 0; i < ids.size(); ++i) s.commit(ids.data()[i]);
      })
      .def("drop", [](SegmentStore& s, Arr<int64_t> ids) {
        for (int64_t i = 0; i < ids.size(); ++i) s.drop(ids.data()[i]);
      })
      .def("pin", [](SegmentStore& s, Arr<int64_t> ids) {
        for (int64_t i = 0; i < ids.size(); ++i) s.pin(ids.data()[i]);
      })
      .def("detach", [](SegmentStore& s, Arr<int64_t> ids) {
        for (int64_t i = 0; i < ids.size(); ++i) s.detach(ids.data()[i]);
      })
      .def("unpin", [](SegmentStore& s, Arr<int64_t> ids) {
        for (int64_t i = 0; i < ids.size(); ++i) s.unpin(ids.data()[i]);
      })
      .def("evict_below", &SegmentStore::evict_below)
      .def("take_delta", [](SegmentStore& s) {
        std::vector<SegKey> add, rm;
        std::vector<int64_t> add_len;
        s.take_delta(&add, &add_len, &rm);
        Arr<int64_t> a({int64_t(add.size()), int64_t(5)}), r({int64_t(rm.size()), int64_t(4)});
        int64_t* ap = a.mutable_data();
        for (size_t i = 0; i < add.size(); ++i) {
          ap[5 * i] = add[i].swarm; ap[5 * i + 1] = add[i].level; ap[5 * i + 2] = add[i].url_id;
          ap[5 * i + 3] = add[i].sn; ap[5 * i + 4] = add_len[i];
        }
        int64_t* rp = r.mutable_data();
        for (size_t i = 0; i < rm.size(); ++i) {
          rp[4 * i] = rm[i].swarm; rp[4 * i + 1] = rm[i].level; rp[4 * i + 2] = rm[i].url_id; rp[4 * i + 3] = rm[i].sn;
        }
        return py::make_tuple(a, r);
      });

  // ------------------------------------------------------------------ directory / planner
  py::class_<Directory>(m, "Directory")
      .def(py::init<>())
      .def_property_readonly("size", &Directory::size)
      // the content digest as a signed 64-bit word (it travels in an int64 control header)
      .def_property_readonly("digest", [](const Directory& d) { return static_cast<int64_t>(d.digest()); })
      .def("apply", [](Directory& d, int rank, Arr<int64_t> adds, Arr<int64_t> removes) {
        // adds int64[n,5] (key4, len); removes int64[m,4]
        for (int64_t i = 0; i < adds.size() / 5; ++i) d.apply_add(rank, key_from(adds.data() + 5 * i), adds.data()[5 * i + 4]);
        for (int64_t i = 0; i < removes.size() / 4; ++i) d.apply_remove(rank, key_from(removes.data() + 4 * i));
      })
      .def("drop_rank", &Directory::drop_rank)
      .def("holder_keys", [](const Directory& d, int rank) {
        // -> int64[n, 5]: key x4, length of the entries `rank` holds
        std::vector<SegKey> k;
        std::vector<int64_t> l;
        d.holder_keys(rank, &k, &l);
        Arr<int64_t> out({int64_t(k.size()), int64_t(5)});
        int64_t* p = out.mutable_data();
        for (size_t i = 0; i < k.size(); ++i) {
          p[5 * i] = k[i].swarm; p[5 * i + 1] = k[i].level; p[5 * i + 2] = k[i].url_id; p[5 * i + 3] = k[i].sn;
          p[5 * i + 4] = l[i];
        }
        return out;
      })
      .def("holders", [](const Directory& d, uint32_t swarm, uint32_t level, uint32_t url_id, uint32_t sn) {
        const DirEntry* e = d.find(SegKey{swarm, level, url_id, sn});
        return e ? e->holders : uint64_t(0);
      });
  // One round's gathered control messages (agent/node.py:_encode layout: header[hdr_words] =
  // magic, flags, #wants, #adds, #removes, leaving, round, cdn, p2p, upload, ...; then wants
  // [key4, size, want_id | force_cdn << 62 | not_staged << 61 | staging << 60 | held << 59], adds [key4, len], removes
  // [key4]) in one call:
  // applies every rank's cache delta to the directory and returns (want rows int64[n, 8] for
  // plan_round, per-rank flags, all-leaving, swarm byte totals [cdn, p2p, upload]).
  //
  // check_word >= 0: header words [check_word, check_word + 3) carry each rank's directory
  // digest taken before this ingest, the digest of the previous round's full plan and that
  // round's number.  They must agree on every rank: otherwise SwarmDivergence is raised
  // before anything is applied, naming the ranks behind each value, so no rank goes on to
  // post a send / receive group its peers do not match (a hang on a two-sided transport).
  m.def("ingest_control", [](Directory& d, const std::vector<Arr<int64_t>>& parts, int64_t magic,
                             int64_t hdr_words, int64_t check_word) {
    const int world = static_cast<int>(parts.size());
    Arr<int64_t> flags(world);
    int64_t tot[3] = {0, 0, 0};
    bool all_leaving = true;
    // pass 1: validate every header (nothing is applied from a round with a bad message) and
    // size the output; pass 2: apply the deltas and write the want rows straight into it
    int64_t n = 0;
    for (int r = 0; r < world; ++r) {
      const int64_t* p = parts[r].data();
      const int64_t size = parts[r].size();
      if (size < hdr_words || p[0] != magic) throw std::runtime_error("bad swarm control message");
      const int64_t nw = p[2], na = p[3], nr = p[4];
      if (nw < 0 || na < 0 || nr < 0 || hdr_words + 6 * nw + 5 * na + 4 * nr > size)
        throw std::runtime_error("truncated swarm control message");
      n += nw;
    }
    if (check_word >= 0 && check_word + 3 <= hdr_words && world > 1) {
      const int64_t* p0 = parts[0].data();
      for (int r = 1; r < world; ++r) {
        const int64_t* p = parts[r].data();
        if (p[check_word] != p0[check_word]) {
          std::ostringstream o;
          o << "swarm directory diverged before round " << p0[6] << " (replica digests "
            << group_ranks(parts, check_word) << ")";
          throw SwarmDivergence(o.str());
        }
        if (p[check_word + 1] != p0[check_word + 1] || p[check_word + 2] != p0[check_word + 2]) {
          std::ostringstream o;
          o << "swarm plans diverged in round " << p0[check_word + 2] << " (plan digests "
            << group_ranks(parts, check_word + 1) << "; planned rounds " << group_ranks(parts, check_word + 2)
            << ")";
          throw SwarmDivergence(o.str());
        }
      }
    }
    Arr<int64_t> out({n, int64_t(8)});
    int64_t* o = out.mutable_data();
    for (int r = 0; r < world; ++r) {
      const int64_t* p = parts[r].data();
      const int64_t nw = p[2], na = p[3], nr = p[4];
      flags.mutable_data()[r] = p[1];
      all_leaving = all_leaving && p[5] != 0;
      tot[0] += p[7];
      tot[1] += p[8];
      tot[2] += p[9];
      const int64_t* w = p + hdr_words;
      const int64_t* a = w + 6 * nw;
      const int64_t* rm = a + 5 * na;
      for (int64_t i = 0; i < na; ++i) d.apply_add(r, key_from(a + 5 * i), a[5 * i + 4]);
      for (int64_t i = 0; i < nr; ++i) d.apply_remove(r, key_from(rm + 4 * i));
      for (int64_t i = 0; i < nw; ++i, o += 8) {
        const int64_t* x = w + 6 * i;
        // want word: want_id | force_cdn << 62 | not_staged << 61 | staging << 60 | held << 59
        // -> WantFlag bits
        o[0] = x[0];
        o[1] = x[1];
        o[2] = x[2];
        o[3] = x[3];
        o[4] = x[4];
        o[5] = x[5] & ((int64_t(1) << 59) - 1);
        o[6] = r;
        o[7] = ((x[5] >> 62) & 1 ? kForceCdn : 0) | ((x[5] >> 61) & 1 ? kNotStaged : 0) |
               ((x[5] >> 60) & 1 ? kStaging : 0) | ((x[5] >> 59) & 1 ? kHeld : 0);
      }
    }
    Arr<int64_t> totals(3);
    std::memcpy(totals.mutable_data(), tot, sizeof(tot));
    return py::make_tuple(out, flags, all_leaving, totals);
  }, py::arg("directory"), py::arg("parts"), py::arg("magic"), py::arg("hdr_words"), py::arg("check_word") = -1);
  // wants: int64[n, 8] = (key4, size, want_id, rank, want_flags); flags int64[world]
  // -> int64[m, 10] = (key4, size, src, dst, want_id, seeded, reserved); src -1 = CDN fetch,
  // -2 = stage (download from a network origin into host memory for a later round)
  // plan_round_for: the same plan, but only the rows this rank takes part in (src == me or
  // dst == me, canonical order kept) plus whether the round has any P2P transfer at all
  // (every rank enters the exchange then) and the 64-bit digest of the full plan (ranks
  // compare it in the next round's control all-gather, see ingest_control).  At 8 ranks a
  // rank needs ~1/4 of the rows: the rest would be built into numpy and masked away in
  // Python every round.
  auto plan_rows = [](const Directory& d, const Arr<int64_t>& wants, const Arr<int64_t>& flags, int world,
                      int me, const py::object& cdn_obj) {
    const int64_t n = wants.size() / 8;
    if (flags.size() != world) throw std::invalid_argument("flags must have world entries");
    std::vector<Want> w(n);
    std::vector<Transfer> t;
    std::vector<int64_t> f;
    const int64_t* p = wants.data();
    for (int64_t i = 0; i < n; ++i) {
      w[i].key = key_from(p + 8 * i);
      w[i].size = p[8 * i + 4];
      w[i].want_id = p[8 * i + 5];
      w[i].rank = static_cast<int32_t>(p[8 * i + 6]);
      w[i].flags = p[8 * i + 7];
      if (w[i].rank < 0 || w[i].rank >= world) throw std::invalid_argument("want rank out of range");
    }
    f.assign(flags.data(), flags.data() + world);
    std::vector<int64_t> cdn;
    if (!cdn_obj.is_none()) {  // each rank's cumulative CDN bytes: the planner's CDN balance
      Arr<int64_t> c = cdn_obj.cast<Arr<int64_t>>();
      if (c.size() != world) throw std::invalid_argument("cdn_bytes must have world entries");
      cdn.assign(c.data(), c.data() + world);
    }
    plan_round_into(d, w.data(), w.size(), f, world, &t, cdn.empty() ? nullptr : cdn.data());
    const int64_t digest = static_cast<int64_t>(plan_digest(t));  // of the FULL plan, before filtering
    bool any_p2p = false;
    int64_t m = 0;
    for (const Transfer& x : t) {
      any_p2p = any_p2p || x.src >= 0;
      if (me < 0 || x.src == me || x.dst == me) ++m;
    }
    Arr<int64_t> out({m, int64_t(10)});
    int64_t* o = out.mutable_data();
    for (const Transfer& x : t) {
      if (me >= 0 && x.src != me && x.dst != me) continue;
      o[0] = x.key.swarm; o[1] = x.key.level; o[2] = x.key.url_id; o[3] = x.key.sn;
      o[4] = x.size; o[5] = x.src; o[6] = x.dst; o[7] = x.want_id; o[8] = x.seeded; o[9] = 0;
      o += 10;
    }
    return std::make_tuple(out, any_p2p, digest);
  };
  m.def("plan_round", [plan_rows](const Directory& d, Arr<int64_t> wants, Arr<int64_t> flags, int world,
                                  py::object cdn_bytes) {
    return std::get<0>(plan_rows(d, wants, flags, world, -1, cdn_bytes));
  }, py::arg("directory"), py::arg("wants"), py::arg("flags"), py::arg("world"), py::arg("cdn_bytes") = py::none());
  m.def("plan_round_for", [plan_rows](const Directory& d, Arr<int64_t> wants, Arr<int64_t> flags, int world,
                                      int me, py::object cdn_bytes) {
    if (me < 0 || me >= world) throw std::invalid_argument("rank out of range");
    auto r = plan_rows(d, wants, flags, world, me, cdn_bytes);
    return py::make_tuple(std::get<0>(r), std::get<1>(r), std::get<2>(r));
  }, py::arg("directory"), py::arg("wants"), py::arg("flags"), py::arg("world"), py::arg("me"),
     py::arg("cdn_bytes") = py::none());
  // CPU-mode CDN phase: copy origin byte ranges (raw host addresses, as the want table holds
  // them) into the node's host arena at `dst_base + dst_off[i]` (bounds-checked against cap)
  m.def("host_copy_batch", [](int64_t dst_base, int64_t dst_cap, Arr<int64_t> dst_off, Arr<int64_t> src_ptr,
                              Arr<int64_t> len) {
    const int64_t n = len.size();
    if (dst_off.size() != n || src_ptr.size() != n) throw std::invalid_argument("host_copy_batch: sizes differ");
    for (int64_t i = 0; i < n; ++i) {
      const int64_t o = dst_off.data()[i], l = len.data()[i];
      if (o < 0 || l < 0 || o + l > dst_cap) throw std::out_of_range("host_copy_batch: destination out of bounds");
      if (l && src_ptr.data()[i] == 0) throw std::invalid_argument("host_copy_batch: null source");
      if (l) std::memcpy(reinterpret_cast<uint8_t*>(dst_base) + o, reinterpret_cast<const uint8_t*>(src_ptr.data()[i]),
                         static_cast<size_t>(l));
    }
  });

  // ------------------------------------------------------------------ want table
  // (agent/node.py: the rank's per-request state as rows; see wants.hpp)
  py::class_<SegmentLocator>(m, "SegmentLocator")
      .def(py::init<>())
      .def("add_dir",
           [](SegmentLocator& l, const std::string& dir, const std::string& prefix, const std::string& suffix,
              int64_t sn_lo, int64_t sn_hi, int64_t base, int64_t flags, Arr<int64_t> off, Arr<int64_t> len) {
             if (off.size() != len.size()) throw std::invalid_argument("add_dir: off / len sizes differ");
             SegmentLocator::Dir d;
             d.prefix = prefix;
             d.suffix = suffix;
             d.sn_lo = sn_lo;
             d.sn_hi = sn_hi;
             d.base = base;
             d.flags = flags;
             d.off.assign(off.data(), off.data() + off.size());
             d.len.assign(len.data(), len.data() + len.size());
             l.add_dir(dir, std::move(d));
           },
           py::arg("dir"), py::arg("prefix"), py::arg("suffix"), py::arg("sn_lo"), py::arg("sn_hi"), py::arg("base"),
           py::arg("flags"), py::arg("off"), py::arg("len"))
      .def("resolve",
           [](const SegmentLocator& l, const py::list& urls) {
             // string views into the list's str objects (the GIL stays held: no other thread
             // can drop an item of the list while the views are in use)
             const size_t n = urls.size();
             std::vector<std::string_view> v(n);
             for (size_t i = 0; i < n; ++i) {
               Py_ssize_t len = 0;
               const char* s = PyUnicode_AsUTF8AndSize(urls[i].ptr(), &len);
               if (s == nullptr) throw py::error_already_set();
               v[i] = std::string_view(s, static_cast<size_t>(len));
             }
             py::array_t<int64_t> size(n), ptr(n), base(n), flags(n);
             py::array_t<uint8_t> ok(n);
             const int64_t found = l.resolve(v, size.mutable_data(), ptr.mutable_data(), base.mutable_data(),
                                             flags.mutable_data(), ok.mutable_data());
             return py::make_tuple(size, ptr, base, flags, ok.attr("astype")("bool"), found);
           })
      .def("clear", &SegmentLocator::clear)
      .def("__len__", &SegmentLocator::size);

  py::class_<WantTable>(m, "WantTable")
      .def(py::init<>())
      .def("__len__", &WantTable::size)
      .def_property_readonly("waiting", &WantTable::waiting)
      .def_property_readonly("num_tokens", &WantTable::tokens)
      .def("add", [](WantTable& t, Arr<int64_t> keys, Arr<int64_t> sizes, Arr<int64_t> ptr, Arr<int64_t> base,
                     Arr<int64_t> flags, Arr<int64_t> tokens) {
        // -> (want ids int64[n], created uint8[n])
        const int64_t n = tokens.size();
        if (keys.size() != 4 * n || sizes.size() != n || ptr.size() != n || base.size() != n || flags.size() != n)
          throw std::invalid_argument("WantTable.add: keys int64[n,4] and n-long columns");
        Arr<int64_t> ids(n);
        Arr<uint8_t> created(n);
        const int64_t* k = keys.data();
        for (int64_t i = 0; i < n; ++i) {
          bool c = false;
          ids.mutable_data()[i] = t.add(key_from(k + 4 * i), sizes.data()[i], ptr.data()[i], base.data()[i],
                                        static_cast<int32_t>(flags.data()[i]), tokens.data()[i], &c);
          created.mutable_data()[i] = c ? 1 : 0;
        }
        return py::make_tuple(ids, created);
      })
      .def("add1", [](WantTable& t, uint32_t swarm, uint32_t level, uint32_t url_id, uint32_t sn, int64_t size,
                      int64_t ptr, int64_t base, int64_t flags, int64_t token) {
        // -> want id, negated - 1 when the want was created (one int back, no tuple)
        bool c = false;
        const int64_t id = t.add(SegKey{swarm, level, url_id, sn}, size, ptr, base, static_cast<int32_t>(flags),
                                 token, &c);
        return c ? -id - 1 : id;
      })
      .def("abort", [](WantTable& t, Arr<int64_t> tokens) {
        int64_t n = 0;
        for (int64_t i = 0; i < tokens.size(); ++i) n += t.abort(tokens.data()[i]) ? 1 : 0;
        return n;
      })
      .def("abort1", &WantTable::abort)
      .def("lookup1", [](const WantTable& t, uint32_t swarm, uint32_t level, uint32_t url_id, uint32_t sn) {
        return t.lookup(SegKey{swarm, level, url_id, sn});
      })
      .def("select", [](WantTable& t, const SegmentStore& store, const Directory* dir, int64_t cap, int32_t round) {
        // -> (admitted ids, control rows int64[k, 6], dropped ids, too-big ids, deferred count)
        std::vector<int64_t> adm, dropped, big;
        int64_t deferred = 0;
        t.select(store, dir, cap, round, &adm, &dropped, &big, &deferred);
        const int64_t k = static_cast<int64_t>(adm.size());
        Arr<int64_t> rows({k, int64_t(6)});
        if (k) t.encode(adm.data(), k, rows.mutable_data());
        auto vec = [](const std::vector<int64_t>& v) {
          Arr<int64_t> a(static_cast<py::ssize_t>(v.size()));
          if (!v.empty()) std::memcpy(a.mutable_data(), v.data(), v.size() * sizeof(int64_t));
          return a;
        };
        return py::make_tuple(vec(adm), rows, vec(dropped), vec(big), deferred);
      }, py::arg("store"), py::arg("directory").none(true), py::arg("cap"), py::arg("round"))
      .def("info", [](const WantTable& t, Arr<int64_t> ids) {
        // -> int64[n, 10]: key x4, size, src_ptr, src_base, flags, round, attempts (row of -1: unknown id)
        const int64_t n = ids.size();
        Arr<int64_t> out({n, int64_t(10)});
        int64_t* o = out.mutable_data();
        for (int64_t i = 0; i < n; ++i, o += 10) {
          const WantRec* r = t.get(ids.data()[i]);
          if (r == nullptr) {
            std::fill(o, o + 10, -1);
            continue;
          }
          o[0] = r->key.swarm; o[1] = r->key.level; o[2] = r->key.url_id; o[3] = r->key.sn;
          o[4] = r->size; o[5] = r->src_ptr; o[6] = r->src_base; o[7] = r->flags; o[8] = r->round;
          o[9] = r->attempts;
        }
        return out;
      })
      .def("set", [](WantTable& t, int64_t id, int64_t size, int64_t set_flags, int64_t clear_flags) {
        // size < 0: unchanged; returns False for an unknown id
        WantRec* r = t.get(id);
        if (r == nullptr) return false;
        if (size >= 0) r->size = size;
        r->flags = static_cast<int32_t>((r->flags | set_flags) & ~clear_flags);
        return true;
      }, py::arg("id"), py::arg("size") = -1, py::arg("set_flags") = 0, py::arg("clear_flags") = 0)
      .def("waiters", [](const WantTable& t, int64_t id) {
        const WantRec* r = t.get(id);
        std::vector<int64_t> w;
        if (r != nullptr) w = r->waiters;
        return w;
      })
      .def("finish", [](WantTable& t, Arr<int64_t> ids) {
        // -> (tokens int64[m], index of each token's want in ids int64[m], prefetch-only uint8[n])
        std::vector<int64_t> tok, idx;
        std::vector<uint8_t> pf;
        t.finish(ids.data(), ids.size(), &tok, &idx, &pf);
        Arr<int64_t> a(static_cast<py::ssize_t>(tok.size())), b(static_cast<py::ssize_t>(idx.size()));
        Arr<uint8_t> c(static_cast<py::ssize_t>(pf.size()));
        if (!tok.empty()) std::memcpy(a.mutable_data(), tok.data(), tok.size() * sizeof(int64_t));
        if (!idx.empty()) std::memcpy(b.mutable_data(), idx.data(), idx.size() * sizeof(int64_t));
        if (!pf.empty()) std::memcpy(c.mutable_data(), pf.data(), pf.size());
        return py::make_tuple(a, b, c);
      })
      .def("requeue", [](WantTable& t, Arr<int64_t> ids, bool force_cdn) { t.requeue(ids.data(), ids.size(), force_cdn); },
           py::arg("ids"), py::arg("force_cdn") = false)
      .def("audit", [](const WantTable& t) {
        std::vector<std::string> e;
        t.audit(&e);
        return e;
      })
      .def("ids", [](const WantTable& t) {
        std::vector<int64_t> v;
        t.ids(&v);
        Arr<int64_t> a(static_cast<py::ssize_t>(v.size()));
        if (!v.empty()) std::memcpy(a.mutable_data(), v.data(), v.size() * sizeof(int64_t));
        return a;
      })
      .def("token_map", [](const WantTable& t) {
        // -> (tokens int64[n], want ids int64[n])
        std::vector<int64_t> tk, w;
        t.token_map(&tk, &w);
        Arr<int64_t> a(static_cast<py::ssize_t>(tk.size())), b(static_cast<py::ssize_t>(w.size()));
        if (!tk.empty()) {
          std::memcpy(a.mutable_data(), tk.data(), tk.size() * sizeof(int64_t));
          std::memcpy(b.mutable_data(), w.data(), w.size() * sizeof(int64_t));
        }
        return py::make_tuple(a, b);
      });
  m.attr("WANT_FORCE_CDN") = int64_t(kWForceCdn);
  m.attr("WANT_NOT_STAGED") = int64_t(kWNotStaged);
  m.attr("WANT_STAGING") = int64_t(kWStaging);
  m.attr("WANT_PREFETCH") = int64_t(kWPrefetch);
  m.attr("WANT_PY") = int64_t(kWPy);
  m.attr("WANT_CORRUPT") = int64_t(kWCorrupt);
  m.attr("WANT_HELD") = int64_t(kWHeld);
  m.attr("WANT_ON_DEV") = int64_t(kWOnDev);
  m.attr("NO_TOKEN") = kNoToken;

  // ------------------------------------------------------------------ intra-node control plane
  py::class_<ShmControl>(m, "ShmControl")
      .def(py::init<const std::string&, int, int, int64_t, bool>(), py::arg("name"), py::arg("rank"),
           py::arg("world"), py::arg("slot_words"), py::arg("create"))
      .def("unlink", &ShmControl::unlink)
      .def_property_readonly("slot_words", &ShmControl::slot_words)
      .def_property_readonly("generation", &ShmControl::generation)
      // all-gather of int64 vectors; None when some rank's message exceeded slot_words
      // (every rank sees the same lengths, so all of them take the caller's fallback)
      .def("allgather",
           [](ShmControl& s, Arr<int64_t> msg, double timeout_s) -> py::object {
             const int64_t n = msg.size();
             {
               py::gil_scoped_release nogil;
               s.exchange(msg.data(), n, timeout_s);
             }
             std::vector<int64_t> lens(s.world());
             for (int r = 0; r < s.world(); ++r) {
               lens[r] = s.length(r);
               if (lens[r] > s.slot_words()) return py::none();
             }
             py::list out;
             for (int r = 0; r < s.world(); ++r) {
               Arr<int64_t> a(static_cast<py::ssize_t>(lens[r]));
               s.read(r, a.mutable_data());
               out.append(a);
             }
             return std::move(out);
           },
           py::arg("msg"), py::arg("timeout_s") = 300.0)
      .def("barrier", [](ShmControl& s, double timeout_s) {
        py::gil_scoped_release nogil;
        s.barrier(timeout_s);
      }, py::arg("timeout_s") = 300.0);

  m.attr("FLAG_ONLINE") = int64_t(kOnline);
  m.attr("FLAG_UPLOAD") = int64_t(kUploadOn);
  m.attr("FLAG_DOWNLOAD") = int64_t(kDownloadOn);
  m.attr("FLAG_CDN_DEDUP") = int64_t(kCdnDedup);
  m.attr("FLAG_CDN_BOUND") = int64_t(kCdnBound);
}
