// The MPEG-TS / PES / NAL / SPS / ADTS byte rules that fill the rows of layout.hpp: the only
// definition of each, called by the host runtime (runtime/ts.cpp, runtime/es.cpp, runtime/remux.cpp,
// runtime/codec.cpp, runtime/sampleaes.cpp, runtime/captions.cpp, runtime/mp4.cpp, runtime/cbcs.cpp,
// runtime/cenc.cpp, runtime/fragment.cpp, runtime/packedaudio.cpp, runtime/mpegaudio.cpp,
// runtime/ac3audio.cpp) and by the gfx950
// kernels (kernels/ts_demux.hip, kernels/es_index.hip, kernels/remux.hip, kernels/fragment.hip, kernels/codec_config.hip,
// kernels/sample_aes.hip, kernels/captions.hip, kernels/mp4_demux.hip, kernels/cbcs.hip, kernels/cenc.hip,
// kernels/packed_audio.hip, kernels/mpeg_audio.hip, kernels/ac3_audio.hip).  Plain inline
// functions over <cstdint> and layout.hpp: no containers, no statics, no tables in memory.
#pragma once
#include <cstdint>

#include "layout.hpp"

#if defined(__HIPCC__)
#define HLSP2P_RULE __host__ __device__ __forceinline__
#else
#define HLSP2P_RULE inline
#endif

namespace hlsp2p {

HLSP2P_RULE int64_t clamp(int64_t v, int64_t lo, int64_t hi) { return v < lo ? lo : v > hi ? hi : v; }

// ---------------------------------------------------------------- MPEG-TS demux
namespace ts {
constexpr int kSync = 0x47;
constexpr int kPusi = 0x40;  // payload_unit_start_indicator, in header byte 1
enum StreamType : int {
  kMpeg1Audio = 0x03, kMpeg2Audio = 0x04, kAdtsAac = 0x0F, kId3 = 0x15, kAvc = 0x1B, kHevc = 0x24,
  kSampleAesAdts = 0xCF, kSampleAesAvc = 0xDB,  // HLS SAMPLE-AES: reported as kAdtsAac / kAvc
  kAc3 = 0x81, kEac3 = 0x87,  // HLS AC-3 / E-AC-3: the audio class only where no AAC / MPEG audio stream took it
};

HLSP2P_RULE int packet_pid(int b1, int b2) { return ((b1 & 0x1f) << 8) | b2; }
HLSP2P_RULE bool has_adaptation(int b3) { return (b3 & 0x20) != 0; }
HLSP2P_RULE bool has_payload(int b3) { return (b3 & 0x10) != 0; }
// first payload byte; b4 (adaptation_field_length) counts only where has_adaptation(b3).
// Past kPacket when the adaptation field is too long.
HLSP2P_RULE int payload_start(int b3, int b4) { return 4 + (has_adaptation(b3) ? 1 + b4 : 0); }

// Offset of the PES header in a packet that starts a payload unit and has room for the header's
// 9 fixed bytes, else -1: the packets whose payload parse_packet reads through hb.
HLSP2P_RULE int pes_header_start(int b0, int b1, int b3, int b4) {
  const int s = payload_start(b3, b4);
  return (b0 == kSync && (b1 & kPusi) && has_payload(b3) && s + 9 <= kPacket) ? s : -1;
}

// Offset of the table_id byte of a section that starts in the 188-byte packet p on `pid`, with at
// least min_bytes of the section inside the packet, else -1.
HLSP2P_RULE int find_section(const uint8_t* p, int pid, int table_id, int min_bytes) {
  if (p[0] != kSync || packet_pid(p[1], p[2]) != pid || !(p[1] & kPusi)) return -1;
  int ps = payload_start(p[3], p[4]);
  if (!has_payload(p[3]) || ps >= kPacket) return -1;
  ps += 1 + p[ps];  // pointer field
  if (ps + min_bytes > kPacket || p[ps] != table_id) return -1;
  return ps;
}

struct Psi {
  int64_t status;  // kNoPat / kNoPmt
  int pmt_pid;     // -1: none
  int pid[kClasses];
  int video_type, audio_type;
};

// PAT -> PMT PID, PMT -> the first ES PID of each class, both within the first kPsiScanPackets
// packets; sections are read as far as they lie inside their first packet.  A Dolby stream (kAc3 /
// kEac3) is a fallback: the first one becomes the audio class behind the walk, if the class is free.
HLSP2P_RULE Psi parse_psi(const uint8_t* data, int64_t n_packets) {
  Psi r = {0, -1, {-1, -1, -1}, 0, 0};
  const int64_t scan = n_packets < kPsiScanPackets ? n_packets : kPsiScanPackets;
  for (int64_t i = 0; i < scan && r.pmt_pid < 0; ++i) {
    const uint8_t* p = data + i * kPacket;
    const int ps = find_section(p, 0, 0x00, 8);
    if (ps < 0) continue;
    const int slen = ((p[ps + 1] & 0x0f) << 8) | p[ps + 2];
    const int end = ps + 3 + slen - 4 < kPacket ? ps + 3 + slen - 4 : kPacket;
    for (int q = ps + 8; q + 4 <= end; q += 4) {
      if (((p[q] << 8) | p[q + 1]) != 0) {  // program 0 is the network PID
        r.pmt_pid = packet_pid(p[q + 2], p[q + 3]);
        break;
      }
    }
  }
  if (r.pmt_pid < 0) r.status |= kNoPat;
  bool pmt_found = false;
  for (int64_t i = 0; i < scan && r.pmt_pid >= 0 && !pmt_found; ++i) {
    const uint8_t* p = data + i * kPacket;
    const int ps = find_section(p, r.pmt_pid, 0x02, 12);
    if (ps < 0) continue;
    pmt_found = true;
    const int slen = ((p[ps + 1] & 0x0f) << 8) | p[ps + 2];
    const int end = ps + 3 + slen - 4 < kPacket ? ps + 3 + slen - 4 : kPacket;
    const int pil = ((p[ps + 10] & 0x0f) << 8) | p[ps + 11];
    int dolby_pid = -1, dolby_type = 0;
    for (int q = ps + 12 + pil; q + 5 <= end;) {
      const int type = p[q];
      const int epid = packet_pid(p[q + 1], p[q + 2]);
      const int eil = ((p[q + 3] & 0x0f) << 8) | p[q + 4];
      if ((type == kAvc || type == kHevc || type == kSampleAesAvc) && r.pid[0] < 0) {
        r.pid[0] = epid;
        r.video_type = type == kSampleAesAvc ? kAvc : type;
      } else if ((type == kAdtsAac || type == kMpeg1Audio || type == kMpeg2Audio || type == kSampleAesAdts) &&
                 r.pid[1] < 0) {
        r.pid[1] = epid;
        r.audio_type = type == kSampleAesAdts ? kAdtsAac : type;
      } else if (type == kId3 && r.pid[2] < 0) {
        r.pid[2] = epid;
      } else if ((type == kAc3 || type == kEac3) && dolby_pid < 0) {
        dolby_pid = epid;
        dolby_type = type;
      }
      q += 5 + eil;
    }
    if (r.pid[1] < 0 && dolby_pid >= 0) {
      r.pid[1] = dolby_pid;
      r.audio_type = dolby_type;
    }
  }
  if (r.pmt_pid >= 0 && !pmt_found) r.status |= kNoPmt;
  return r;
}

// the 33-bit PTS / DTS whose 5 bytes start at byte i of hb
template <class HB>
HLSP2P_RULE int64_t read_ts33(HB hb, int i) {
  return (int64_t((hb(i) >> 1) & 0x07) << 30) | (int64_t(hb(i + 1)) << 22) | (int64_t(hb(i + 2) >> 1) << 15) |
         (int64_t(hb(i + 3)) << 7) | int64_t(hb(i + 4) >> 1);
}

struct Packet {
  int cls;         // kClasses: the packet carries no ES bytes
  int start, len;  // ES bytes inside the packet
  int pes;         // 1: the packet starts a PES with these stamps (-1 = absent)
  int64_t pts, dts;
  int err;  // kBadSync / kBadLength / kPesHeaderError: counted in the status, the packet is dropped
};

// One packet from its first five bytes (b4 counts only with an adaptation field), the ES PIDs of
// the three classes (-1 = none) and hb(i), byte i of the payload, which is asked only for
// i < min(payload length, 19).
template <class HB>
HLSP2P_RULE Packet parse_packet(int b0, int b1, int b2, int b3, int b4, int vpid, int apid, int ipid, HB hb) {
  Packet r = {kClasses, 0, 0, 0, -1, -1, 0};
  if (b0 != kSync) {
    r.err = static_cast<int>(kBadSync);
    return r;
  }
  const int pid = packet_pid(b1, b2);
  const int cls = (vpid >= 0 && pid == vpid) ? 0 : (apid >= 0 && pid == apid) ? 1 : (ipid >= 0 && pid == ipid) ? 2 : kClasses;
  if (cls == kClasses || !has_payload(b3)) return r;
  int s = payload_start(b3, b4);
  if (s > kPacket) {
    r.err = static_cast<int>(kBadLength);
    return r;
  }
  int l = kPacket - s;
  if (b1 & kPusi) {
    if (l < 9 || hb(0) != 0 || hb(1) != 0 || hb(2) != 1 || 9 + hb(8) > l) {
      r.err = static_cast<int>(kPesHeaderError);
      return r;
    }
    const int flags = hb(7);
    if ((flags & 0x80) && l >= 14) r.pts = read_ts33(hb, 9);
    if ((flags & 0xC0) == 0xC0 && l >= 19) r.dts = read_ts33(hb, 14);
    r.pes = 1;
    s += 9 + hb(8);
    l -= 9 + hb(8);
  }
  r.cls = cls;
  r.start = s;
  r.len = l;
  return r;
}
}  // namespace ts

// ---------------------------------------------------------------- sample index
namespace es {
HLSP2P_RULE bool video_supported(int64_t vtype) { return vtype == ts::kAvc || vtype == ts::kHevc; }
HLSP2P_RULE bool is_hevc(int64_t vtype) { return vtype == ts::kHevc; }
HLSP2P_RULE bool is_adts(int64_t atype) { return atype == ts::kAdtsAac; }
HLSP2P_RULE int nal_type(bool hevc, int byte) { return hevc ? (byte >> 1) & 0x3f : byte & 0x1f; }

// ---- one demuxed segment as the index and the remux read it: damaged info rows are clamped
// here, once, so host and device agree byte for byte
struct Segment {
  const uint8_t* es;  // [video ES | audio ES | id3 ES]
  int64_t cap;        // readable bytes of es; the caller decides how far it trusts the value
  const int64_t *info, *pes;
  int64_t max_pes, max_nal;
};
// segment b of a batch
HLSP2P_RULE Segment segment_at(const uint8_t* es, const int64_t* es_off, const int64_t* cap, const int64_t* info,
                               const int64_t* pes, int64_t max_pes, int64_t max_nal, int64_t b) {
  return {es + es_off[b], cap[b], info + b * ts::kInfoWords, pes + ts::pes_words(b, max_pes), max_pes, max_nal};
}
template <class I32, class I64>
HLSP2P_RULE IndexTables<I32, I64> index_tables_at(const IndexTables<I32, I64>& t, const Segment& s, int64_t b) {
  return {t.nal + table_words(b, s.max_nal, kNalWords), t.au + table_words(b, s.max_pes, kAuWords),
          t.aframes + table_words(b, s.max_pes, kApesWords), t.sinfo + b * kSinfoWords};
}
HLSP2P_RULE RemuxTables remux_tables_at(const RemuxTables& t, const Segment& s, int64_t max_aframes, int64_t b) {
  return {t.vsamples + table_words(b, s.max_pes, kVsampleWords), t.asamples + table_words(b, max_aframes, kAsampleWords),
          t.rinfo + b * kRinfoWords};
}

struct PesRows { const int64_t *video, *audio; };
HLSP2P_RULE PesRows pes_rows(const Segment& s) { return {s.pes, s.pes + table_words(1, s.max_pes, ts::kPesWords)}; }
HLSP2P_RULE int64_t pes_at(const int64_t* rows, int64_t k, ts::PesRow col) { return rows[ts::kPesWords * k + col]; }

struct VideoSpan {
  bool supported, hevc;
  int64_t len;  // video ES bytes to read: 0 for an unsupported codec, never beyond cap
};
HLSP2P_RULE VideoSpan video_span(const int64_t* info, int64_t cap) {
  const int64_t vtype = info[ts::kVideoType];
  const bool supported = video_supported(vtype);
  return {supported, is_hevc(vtype), supported ? clamp(info[ts::kVideoBytes], 0, cap) : 0};
}
HLSP2P_RULE VideoSpan video_span(const Segment& s) { return video_span(s.info, s.cap); }
// rows of a video table (NALs, access units) among `count` claimed ones: an unsupported codec has none
HLSP2P_RULE int64_t video_rows(const VideoSpan& v, int64_t count, int64_t max_rows) {
  return v.supported ? clamp(count, 0, max_rows) : 0;
}

struct AudioSpan {
  int64_t off, len;  // the audio ES inside es
  int64_t n_pes;     // rows of the audio PES table
  int64_t n_adts;    // the same, 0 unless the stream is ADTS: the PES whose frames are walked
};
HLSP2P_RULE AudioSpan audio_span(const Segment& s) {
  const int64_t off = clamp(s.info[ts::kAudioEsOffset], 0, s.cap);
  const int64_t n_pes = clamp(s.info[ts::kNumAudioPes], 0, s.max_pes);
  return {off, clamp(s.info[ts::kAudioBytes], 0, s.cap - off), n_pes, is_adts(s.info[ts::kAudioType]) ? n_pes : 0};
}
// bytes [start, end) of the audio ES that audio PES k < a.n_adts covers: up to the next PES, inside the ES
struct ByteRange { int64_t start, end; };
HLSP2P_RULE ByteRange audio_pes_range(const int64_t* ap, int64_t k, const AudioSpan& a) {
  const int64_t start = clamp(pes_at(ap, k, ts::kPesEsOffset), 0, a.len);
  return {start, k + 1 < a.n_adts ? clamp(pes_at(ap, k + 1, ts::kPesEsOffset), start, a.len) : a.len};
}

HLSP2P_RULE int nal_flags(bool hevc, int type) {
  if (hevc)
    return (type >= 16 && type <= 21 ? kAuKeyframe : 0) | (type == 33 ? kAuSps : 0) | (type == 34 ? kAuPps : 0) |
           (type == 35 ? kAuAud : 0);
  return (type == 5 ? kAuKeyframe : 0) | (type == 7 ? kAuSps : 0) | (type == 8 ? kAuPps : 0) | (type == 9 ? kAuAud : 0);
}

HLSP2P_RULE int adts_rate(int idx) {
  switch (idx) {
    case 0: return 96000; case 1: return 88200; case 2: return 64000; case 3: return 48000;
    case 4: return 44100; case 5: return 32000; case 6: return 24000; case 7: return 22050;
    case 8: return 16000; case 9: return 12000; case 10: return 11025; case 11: return 8000;
    case 12: return 7350; default: return 0;
  }
}

struct AdtsWalk {
  int32_t frames, used;  // whole frames, and their bytes
  bool error;            // the walk stopped at bytes that are no frame inside [start, end)
};

// The ADTS frames of one audio PES, bytes [start, end) of the audio ES A.  The first frame of the
// segment's first PES gives the sample rate and the channel configuration.
HLSP2P_RULE AdtsWalk adts_walk(const uint8_t* A, int64_t start, int64_t end, bool first_pes, int& rate, int& chans) {
  AdtsWalk r = {0, 0, false};
  int64_t q = start;
  while (q != end) {
    if (q + 7 > end || A[q] != 0xFF || (A[q + 1] & 0xF6) != 0xF0) {
      r.error = true;
      break;
    }
    const int64_t len = (int64_t(A[q + 3] & 3) << 11) | (int64_t(A[q + 4]) << 3) | (A[q + 5] >> 5);
    const int hdr = (A[q + 1] & 1) ? 7 : 9;
    if (len < hdr || q + len > end) {
      r.error = true;
      break;
    }
    if (first_pes && r.frames == 0) {
      rate = adts_rate((A[q + 2] >> 2) & 15);
      chans = ((A[q + 2] & 1) << 2) | (A[q + 3] >> 6);
    }
    ++r.frames;
    q += len;
  }
  r.used = static_cast<int32_t>(q - start);
  return r;
}

// ---- remux (docs/REMUX.md)
// NAL types that go into an fMP4 sample.  H.264: slices, SEI, SPS, PPS (what hls.js pushes);
// HEVC: everything but AUD, end of sequence, end of bitstream and filler data.
HLSP2P_RULE bool nal_kept(bool hevc, int type) {
  if (hevc) return type >= 0 && (type < 35 || type > 38);
  return type == 1 || type == 5 || type == 6 || type == 7 || type == 8;
}

struct AdtsFrame {
  int32_t len, hdr;  // whole frame and its header; len == 0: no frame at q
};
// The frame adts_walk would count at q of [.., end): the same sync, length and header rule.
HLSP2P_RULE AdtsFrame adts_frame_at(const uint8_t* A, int64_t q, int64_t end) {
  if (q + 7 > end || A[q] != 0xFF || (A[q + 1] & 0xF6) != 0xF0) return {0, 0};
  const int32_t len = (int32_t(A[q + 3] & 3) << 11) | (int32_t(A[q + 4]) << 3) | (A[q + 5] >> 5);
  const int32_t hdr = (A[q + 1] & 1) ? 7 : 9;
  if (len < hdr || q + len > end) return {0, 0};
  return {len, hdr};
}

// ---- codec configuration (docs/INITSEGMENT.md)
// The three ADTS header fields an AudioSpecificConfig is made of, from the frame at q.
struct AdtsConfig { int32_t object_type, rate_index, channel_config; };
HLSP2P_RULE AdtsConfig adts_config_at(const uint8_t* A, int64_t q) {
  return {((A[q + 2] >> 6) & 3) + 1, (A[q + 2] >> 2) & 15, ((A[q + 2] & 1) << 2) | (A[q + 3] >> 6)};
}
HLSP2P_RULE bool adts_config_usable(const AdtsConfig& c) { return c.rate_index < 13 && c.channel_config != 0; }

// ---- MPEG audio frames (docs/MPEGAUDIO.md)
HLSP2P_RULE bool is_mpeg_audio(int64_t atype) { return atype == ts::kMpeg1Audio || atype == ts::kMpeg2Audio; }
// kbit/s of bitrate index bi = 1..14; v1: MPEG-1, else MPEG-2 / 2.5; layer 1..3
HLSP2P_RULE int mpa_kbps(bool v1, int layer, int bi) {
  if (v1 && layer == 1) return 32 * bi;
  if (v1 && layer == 2) {
    switch (bi) {
      case 1: return 32; case 2: return 48; case 3: return 56; case 4: return 64; case 5: return 80;
      case 6: return 96; case 7: return 112; case 8: return 128; case 9: return 160; case 10: return 192;
      case 11: return 224; case 12: return 256; case 13: return 320; default: return 384;
    }
  }
  if (v1) {
    switch (bi) {
      case 1: return 32; case 2: return 40; case 3: return 48; case 4: return 56; case 5: return 64;
      case 6: return 80; case 7: return 96; case 8: return 112; case 9: return 128; case 10: return 160;
      case 11: return 192; case 12: return 224; case 13: return 256; default: return 320;
    }
  }
  if (layer == 1) {
    switch (bi) {
      case 1: return 32; case 2: return 48; case 3: return 56; case 4: return 64; case 5: return 80;
      case 6: return 96; case 7: return 112; case 8: return 128; case 9: return 144; case 10: return 160;
      case 11: return 176; case 12: return 192; case 13: return 224; default: return 256;
    }
  }
  switch (bi) {
    case 1: return 8; case 2: return 16; case 3: return 24; case 4: return 32; case 5: return 40;
    case 6: return 48; case 7: return 56; case 8: return 64; case 9: return 80; case 10: return 96;
    case 11: return 112; case 12: return 128; case 13: return 144; default: return 160;
  }
}

struct MpaFrame {
  int32_t len;      // whole frame, header included; 0: no header at q
  bool counts;      // the frame ends inside [.., end)
  int32_t key;      // (V, L, ri, mono) packed: what every frame of a segment has in common
  int32_t samples, rate, channels, version, layer, bitrate;  // version 1, 2 or 25; bitrate in bit/s
};
// The header in bytes b1 b2 b3 behind a first byte FF, whatever lies behind it.
HLSP2P_RULE MpaFrame mpa_header(int b1, int b2, int b3) {
  MpaFrame f = {0, false, 0, 0, 0, 0, 0, 0, 0};
  const int V = (b1 >> 3) & 3, L = (b1 >> 1) & 3, bi = b2 >> 4, ri = (b2 >> 2) & 3, pad = (b2 >> 1) & 1;
  if ((b1 & 0xE0) != 0xE0 || V == 1 || L == 0 || bi == 0 || bi == 15 || ri == 3) return f;
  const bool v1 = V == 3;
  const int mono = (b3 >> 6) == 3;
  f.layer = 4 - L;
  f.version = v1 ? 1 : V == 2 ? 2 : 25;
  f.rate = (ri == 0 ? 44100 : ri == 1 ? 48000 : 32000) >> (v1 ? 0 : V == 2 ? 1 : 2);
  f.bitrate = 1000 * mpa_kbps(v1, f.layer, bi);
  f.channels = mono ? 1 : 2;
  f.key = (V << 5) | (L << 3) | (ri << 1) | mono;
  if (f.layer == 1) {
    f.len = (12 * f.bitrate / f.rate + pad) * 4;
    f.samples = 384;
  } else if (f.layer == 2 || v1) {
    f.len = 144 * f.bitrate / f.rate + pad;
    f.samples = 1152;
  } else {
    f.len = 72 * f.bitrate / f.rate + pad;
    f.samples = 576;
  }
  return f;
}
// The frame at q of [.., end): len == 0 without a header there (q + 4 <= end, FF and the field rules).
HLSP2P_RULE MpaFrame mpa_frame_at(const uint8_t* A, int64_t q, int64_t end) {
  if (q + 4 > end || A[q] != 0xFF) return {0, false, 0, 0, 0, 0, 0, 0, 0};
  MpaFrame f = mpa_header(A[q + 1], A[q + 2], A[q + 3]);
  f.counts = f.len > 0 && q + f.len <= end;
  return f;
}
// bytes [start, end) of the audio ES that audio PES k < a.n_pes covers: up to the next PES, inside the ES
HLSP2P_RULE ByteRange mpa_pes_range(const int64_t* ap, int64_t k, const AudioSpan& a) {
  const int64_t start = clamp(pes_at(ap, k, ts::kPesEsOffset), 0, a.len);
  return {start, k + 1 < a.n_pes ? clamp(pes_at(ap, k + 1, ts::kPesEsOffset), start, a.len) : a.len};
}
// The audio box offset the MPEG audio op trusts: rinfo's, with the box header inside the region
HLSP2P_RULE int64_t mpa_audio_box(int64_t a0, int64_t region) { return clamp(a0, 0, region > 8 ? region - 8 : 0); }

struct MpaWalk {
  int32_t frames, used;  // whole frames with the segment's key, and their bytes
  bool error;            // the walk stopped in front of the PES's end
  bool format_change;    // the PES starts with a header of another key: nothing of it counts
};
// The frames of one audio PES, bytes [start, end) of the audio ES: back to back, each with `key`.
// fa(q, end) is the codec's frame rule (mpa_frame_at, ac3_frame_at) on the caller's bytes: any type
// with len, counts and key; on_frame(j, q, len) sees every counted frame.
template <class FA, class F>
HLSP2P_RULE MpaWalk mpa_walk(FA&& fa, int64_t start, int64_t end, int32_t key, F&& on_frame) {
  MpaWalk r = {0, 0, false, false};
  int64_t q = start;
  while (q != end) {
    const auto f = fa(q, end);
    if (r.frames == 0 && f.len > 0 && f.key != key) {
      r.format_change = true;
      return r;
    }
    if (!f.counts || f.key != key) {
      r.error = true;
      break;
    }
    on_frame(r.frames, q, f.len);
    ++r.frames;
    q += f.len;
  }
  r.used = static_cast<int32_t>(q - start);
  return r;
}

// ---- AC-3 / E-AC-3 frames (docs/AC3AUDIO.md): ATSC A/52 syncinfo and bsi, Table 5.18, Annex E
HLSP2P_RULE bool is_dolby_audio(int64_t atype) { return atype == ts::kAc3 || atype == ts::kEac3; }
// kbit/s of bit_rate_code i = 0..18 (frmsizecod >> 1)
HLSP2P_RULE int ac3_kbps(int i) {
  switch (i) {
    case 0: return 32; case 1: return 40; case 2: return 48; case 3: return 56; case 4: return 64;
    case 5: return 80; case 6: return 96; case 7: return 112; case 8: return 128; case 9: return 160;
    case 10: return 192; case 11: return 224; case 12: return 256; case 13: return 320; case 14: return 384;
    case 15: return 448; case 16: return 512; case 17: return 576; default: return 640;
  }
}
HLSP2P_RULE int ac3_rate(int fscod) { return fscod == 0 ? 48000 : fscod == 1 ? 44100 : 32000; }
HLSP2P_RULE int ac3_channels(int acmod, int lfeon) {
  switch (acmod) {
    case 0: return 2 + lfeon; case 1: return 1 + lfeon; case 2: return 2 + lfeon; case 3: return 3 + lfeon;
    case 4: return 3 + lfeon; case 5: return 4 + lfeon; case 6: return 4 + lfeon; default: return 5 + lfeon;
  }
}

struct Ac3Frame {
  int32_t len;     // whole syncframe; 0: no header at q
  bool counts;     // a supported layout, and the frame ends inside [.., end)
  int32_t key;     // (kind, fscod, acmod, lfeon, bsid) packed; kAc3NoKey where the layout is unsupported
  bool layout_ok;  // false: a valid E-AC-3 header of a layout that is out of scope
  int32_t kind;    // kAc3KindAc3 / kAc3KindEac3
  int32_t rate, channels, bsid, bitrate, fscod, bsmod, acmod, lfeon, bit_rate_code, data_rate;
};
// The header in bytes b2 .. b6 behind the syncword 0B 77, whatever lies behind it.
HLSP2P_RULE Ac3Frame ac3_header(int b2, int b3, int b4, int b5, int b6) {
  Ac3Frame f = {0, false, kAc3NoKey, false, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  const int bsid = b5 >> 3;
  if (bsid <= 8) {
    const int fscod = b4 >> 6, code = b4 & 0x3F;
    if (fscod == 3 || code > 37) return f;
    const int kbps = ac3_kbps(code >> 1);
    const int words = fscod == 0 ? 2 * kbps : fscod == 1 ? kbps * 320 / 147 + (code & 1) : 3 * kbps;
    const int acmod = b6 >> 5;
    const int skip = 2 * ((acmod & 1) && acmod != 1) + 2 * ((acmod & 4) != 0) + 2 * (acmod == 2);
    f.len = 2 * words;
    f.layout_ok = true;
    f.kind = kAc3KindAc3;
    f.fscod = fscod;
    f.bsmod = b5 & 7;
    f.acmod = acmod;
    f.lfeon = (b6 >> (4 - skip)) & 1;
    f.bit_rate_code = code >> 1;
    f.bitrate = 1000 * kbps;
  } else if (bsid >= 11 && bsid <= 16) {
    const int strmtyp = b2 >> 6, substreamid = (b2 >> 3) & 7, frmsiz = ((b2 & 7) << 8) | b3;
    const int fscod = b4 >> 6, numblkscod = (b4 >> 4) & 3;
    if (2 * (frmsiz + 1) < 8) return f;
    f.len = 2 * (frmsiz + 1);
    f.kind = kAc3KindEac3;
    f.layout_ok = strmtyp == 0 && substreamid == 0 && fscod != 3 && numblkscod == 3;
    if (!f.layout_ok) return f;
    f.fscod = fscod;
    f.acmod = (b4 >> 1) & 7;
    f.lfeon = b4 & 1;
    f.bitrate = 8 * f.len * ac3_rate(fscod) / kAc3FrameSamples;
    f.data_rate = f.bitrate / 1000;
  } else {
    return f;
  }
  f.bsid = bsid;
  f.rate = ac3_rate(f.fscod);
  f.channels = ac3_channels(f.acmod, f.lfeon);
  f.key = (f.kind << 13) | (f.fscod << 11) | (f.acmod << 6) | (f.lfeon << 5) | bsid;
  return f;
}
// The frame at q of [.., end): len == 0 without a header there (q + 7 <= end, 0B 77 and the bsid's rule).
HLSP2P_RULE Ac3Frame ac3_frame_at(const uint8_t* A, int64_t q, int64_t end) {
  if (q + 7 > end || A[q] != 0x0B || A[q + 1] != 0x77)
    return {0, false, kAc3NoKey, false, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  Ac3Frame f = ac3_header(A[q + 2], A[q + 3], A[q + 4], A[q + 5], A[q + 6]);
  f.counts = f.layout_ok && q + f.len <= end;
  return f;
}
// The ac3info row of a segment with a config, whose audio PES 0 starts with `first`, and its row in
// mpainfo's layout (version and layer stay 0: fragment_moof takes the rate and the frame samples).
HLSP2P_RULE void ac3_info_row(int64_t* row, int64_t status, int64_t n_frames, const Ac3Frame& first) {
  row[kAcStatus] = status;
  row[kAcNumFrames] = n_frames;
  row[kAcSampleRate] = first.rate;
  row[kAcChannels] = first.channels;
  row[kAcKind] = first.kind;
  row[kAcBsid] = first.bsid;
  row[kAcFrameSamples] = kAc3FrameSamples;
  row[kAcBitrate] = first.bitrate;
  row[kAcFscod] = first.fscod;
  row[kAcBsmod] = first.bsmod;
  row[kAcAcmod] = first.acmod;
  row[kAcLfeon] = first.lfeon;
  row[kAcBitRateCode] = first.bit_rate_code;
  row[kAcDataRate] = first.data_rate;
  row[kAcFirstFrameBytes] = first.len;
  row[kAcSpare] = 0;
}
HLSP2P_RULE void ac3_mpainfo_row(int64_t* row, int64_t n_frames, const Ac3Frame& first) {
  row[kMpStatus] = 0;
  row[kMpNumFrames] = n_frames;
  row[kMpSampleRate] = first.rate;
  row[kMpChannels] = first.channels;
  row[kMpVersion] = 0;
  row[kMpLayer] = 0;
  row[kMpFrameSamples] = kAc3FrameSamples;
  row[kMpBitrate] = first.bitrate;
}

// Byte j >= 2 of a NAL unit is an emulation-prevention byte iff it is 03 behind two raw zeros
// (p2 = b[j - 2], p1 = b[j - 1], b = b[j]).  Equal to the sequential rule: a dropped byte is never zero.
HLSP2P_RULE bool is_emulation_prevention(int p2, int p1, int b) { return b == 3 && p1 == 0 && p2 == 0; }

// ---- HLS SAMPLE-AES (docs/SAMPLEAES.md)
// NAL row of an H.264 video ES with m access units: a slice (type 1 or 5) of an access unit the
// remux keeps, with n > 0 clamped bytes, is unescaped and measured.
HLSP2P_RULE bool sample_nal_candidate(int type, int64_t au, int64_t m, int64_t n) {
  return (type == 1 || type == 5) && au >= 0 && au < m && n > 0;
}
// A candidate of u unescaped bytes is protected iff it is longer than the clear lead plus one block.
HLSP2P_RULE bool sample_nal_protected(int64_t u) { return u > kSaClearLead + kAesBlock; }
// Block j = 0, 1, .. of a protected NAL starts here in the unescaped NAL ...
HLSP2P_RULE int64_t sample_block_at(int64_t j) { return kSaClearLead + kSaBlockStride * j; }
// ... and is a cipher block iff more than 16 bytes remain at its start (strictly: a block that
// ends exactly at u stays clear).
HLSP2P_RULE bool sample_is_cipher_block(int64_t j, int64_t u) { return sample_block_at(j) + kAesBlock < u; }
// cipher blocks of a NAL of u unescaped bytes
HLSP2P_RULE int64_t sample_video_blocks(int64_t u) {
  return sample_nal_protected(u) ? (u - kSaClearLead - kAesBlock - 1) / kSaBlockStride + 1 : 0;
}
// Cipher blocks of an ADTS frame, back to back from q + hdr + kSaAudioLead: the whole blocks of
// the payload behind the 16-byte leader, none for a payload below 32 bytes.
HLSP2P_RULE int64_t sample_audio_blocks(const AdtsFrame& f) {
  const int64_t payload = f.len - f.hdr;
  return payload < kSaAudioLead + kAesBlock ? 0 : (payload - kSaAudioLead) / kAesBlock;
}
// The status bits of a segment, from its demux and index rows alone.
HLSP2P_RULE int64_t sample_status(const Segment& s, const int64_t* sinfo) {
  const int64_t vtype = s.info[ts::kVideoType];
  int64_t st = 0;
  if (sinfo[kStatus] & kNalOverflow) st |= kSaTruncated;
  if (vtype != ts::kAvc && clamp(s.info[ts::kVideoBytes], 0, s.cap) > 0) st |= kSaUnsupportedVideo;
  if (!is_adts(s.info[ts::kAudioType]) && clamp(s.info[ts::kNumAudioPes], 0, s.max_pes) > 0) st |= kSaUnsupportedAudio;
  if (sinfo[kStatus] & kAdtsError) st |= kSaPartialAudio;
  return st;
}

// What sps_parse reads, in the order of the cinfo row (Cinfo kCProfileIdc .. kCSarHeight).
struct SpsFields {
  int32_t profile_idc, profile_compat, level_idc;
  int32_t chroma_format_idc, bit_depth_luma, bit_depth_chroma, width, height, sar_width, sar_height;
};
constexpr int kSpsFieldWords = 10;
static_assert(sizeof(SpsFields) == kSpsFieldWords * sizeof(int32_t) && kCSarHeight - kCProfileIdc + 1 == kSpsFieldWords,
              "SpsFields is the cinfo row's kCProfileIdc .. kCSarHeight");

// Most-significant-bit-first reader over RBSP bytes rb(0 .. n); a read past the end or a ue
// with more than 31 leading zeros sets err and yields 0 from then on.
template <class RB>
struct SpsBits {
  RB rb;
  int64_t nbits, pos;
  bool err;
  HLSP2P_RULE uint32_t u(int k) {
    uint32_t v = 0;
    for (int i = 0; i < k; ++i) {
      if (err || pos >= nbits) {
        err = true;
        return 0;
      }
      v = (v << 1) | ((static_cast<uint32_t>(rb(pos >> 3)) >> (7 - (pos & 7))) & 1u);
      ++pos;
    }
    return v;
  }
  HLSP2P_RULE uint32_t ue() {
    int z = 0;
    while (!err && u(1) == 0 && !err) {
      if (++z > 31) err = true;
    }
    if (err) return 0;
    const uint32_t rest = u(z);
    return err ? 0 : ((uint32_t(1) << z) - 1u) + rest;  // z <= 31: at most 2^32 - 2
  }
  HLSP2P_RULE int64_t se() {
    const int64_t k = ue();
    return (k & 1) ? (k + 1) / 2 : -(k / 2);
  }
};

HLSP2P_RULE bool sps_high_profile(uint32_t p) {
  return p == 100 || p == 110 || p == 122 || p == 244 || p == 44 || p == 83 || p == 86 || p == 118 || p == 128 ||
         p == 138 || p == 139 || p == 134 || p == 135;
}
// the sample aspect ratio of aspect_ratio_idc 1..16 as (width << 16) | height, 0 for any other idc
HLSP2P_RULE uint32_t sps_sar(uint32_t idc) {
  switch (idc) {
    case 1: return (1u << 16) | 1; case 2: return (12u << 16) | 11; case 3: return (10u << 16) | 11;
    case 4: return (16u << 16) | 11; case 5: return (40u << 16) | 33; case 6: return (24u << 16) | 11;
    case 7: return (20u << 16) | 11; case 8: return (32u << 16) | 11; case 9: return (80u << 16) | 33;
    case 10: return (18u << 16) | 11; case 11: return (15u << 16) | 11; case 12: return (64u << 16) | 33;
    case 13: return (160u << 16) | 99; case 14: return (4u << 16) | 3; case 15: return (3u << 16) | 2;
    case 16: return (2u << 16) | 1; default: return 0;
  }
}

// An H.264 sequence parameter set from its RBSP (the NAL without header byte and emulation
// prevention): rb(i) is RBSP byte i < n.  false: an error (docs/INITSEGMENT.md lists them); f then
// keeps profile_idc / profile_compat / level_idc as read (0 with n < 3) and 0 in every other field.
// Every loop is bounded by a constant or consumes input, so any bytes terminate.
template <class RB>
HLSP2P_RULE bool sps_parse(RB rb, int64_t n, SpsFields& f) {
  f = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  if (n < 3) return false;
  SpsBits<RB> r = {rb, 8 * n, 0, false};
  const uint32_t profile = r.u(8);
  f.profile_idc = static_cast<int32_t>(profile);
  f.profile_compat = static_cast<int32_t>(r.u(8));
  f.level_idc = static_cast<int32_t>(r.u(8));
  r.ue();  // seq_parameter_set_id
  uint32_t chroma = 1, depth_luma = 0, depth_chroma = 0, separate = 0;
  if (sps_high_profile(profile)) {
    chroma = r.ue();
    if (r.err || chroma > 3) return false;
    if (chroma == 3) separate = r.u(1);
    depth_luma = r.ue();
    depth_chroma = r.ue();
    if (r.err || depth_luma > 6 || depth_chroma > 6) return false;
    r.u(1);  // qpprime_y_zero_transform_bypass
    if (r.u(1)) {  // seq_scaling_matrix_present
      const int lists = chroma == 3 ? 12 : 8;
      for (int l = 0; l < lists && !r.err; ++l) {
        if (!r.u(1)) continue;
        const int entries = l < 6 ? 16 : 64;
        int64_t last = 8, next = 8;
        for (int e = 0; e < entries && !r.err; ++e) {
          if (next != 0) next = (((last + r.se()) % 256) + 256) % 256;
          last = next ? next : last;
        }
      }
    }
  }
  r.ue();  // log2_max_frame_num_minus4
  const uint32_t poc_type = r.ue();
  if (r.err) return false;
  if (poc_type == 0) {
    r.ue();
  } else if (poc_type == 1) {
    r.u(1);
    r.se();
    r.se();
    const uint32_t cycle = r.ue();
    if (r.err || cycle > 255) return false;
    for (uint32_t i = 0; i < cycle && !r.err; ++i) r.se();
  }
  r.ue();  // max_num_ref_frames
  r.u(1);  // gaps_in_frame_num_value_allowed
  const int64_t W = r.ue(), H = r.ue();
  const int64_t F = r.u(1);
  if (!F) r.u(1);  // mb_adaptive_frame_field
  r.u(1);          // direct_8x8_inference
  int64_t left = 0, right = 0, top = 0, bottom = 0;
  if (r.u(1)) {  // frame_cropping
    left = r.ue();
    right = r.ue();
    top = r.ue();
    bottom = r.ue();
  }
  uint32_t sar_w = 1, sar_h = 1;
  if (r.u(1) && r.u(1)) {  // vui_parameters_present, aspect_ratio_info_present
    const uint32_t idc = r.u(8);
    uint32_t w = sps_sar(idc) >> 16, h = sps_sar(idc) & 0xffff;
    if (idc == 255) {
      w = r.u(16);
      h = r.u(16);
    }
    if (w != 0 && h != 0) {
      sar_w = w;
      sar_h = h;
    }
  }
  if (r.err) return false;
  const bool planes = chroma == 0 || separate != 0;
  const int64_t cx = planes ? 1 : chroma == 3 ? 1 : 2;
  const int64_t cy = (2 - F) * (planes ? 1 : chroma == 1 ? 2 : 1);
  const int64_t width = 16 * (W + 1) - cx * (left + right);
  const int64_t height = 16 * (2 - F) * (H + 1) - cy * (top + bottom);
  if (width < 1 || width > 65535 || height < 1 || height > 65535) return false;
  f.chroma_format_idc = static_cast<int32_t>(chroma);
  f.bit_depth_luma = static_cast<int32_t>(8 + depth_luma);
  f.bit_depth_chroma = static_cast<int32_t>(8 + depth_chroma);
  f.width = static_cast<int32_t>(width);
  f.height = static_cast<int32_t>(height);
  f.sar_width = static_cast<int32_t>(sar_w);
  f.sar_height = static_cast<int32_t>(sar_h);
  return true;
}

// What hevc_sps_parse reads, in the order of the hinfo row (Hinfo kHProfileSpace .. kHHeight).
// profile_compat holds the 32 general_profile_compatibility_flags as a bit pattern (flag 0 is bit
// 31), constraint_hi / constraint_lo the upper 16 and lower 32 of the 48 constraint-indicator bits.
struct HevcSpsFields {
  int32_t profile_space, tier_flag, profile_idc, profile_compat, constraint_hi, constraint_lo, level_idc;
  int32_t num_temporal_layers, temporal_id_nested, chroma_format_idc, bit_depth_luma, bit_depth_chroma, width, height;
};
constexpr int kHevcSpsFieldWords = 14;
static_assert(sizeof(HevcSpsFields) == kHevcSpsFieldWords * sizeof(int32_t) &&
                  kHHeight - kHProfileSpace + 1 == kHevcSpsFieldWords,
              "HevcSpsFields is the hinfo row's kHProfileSpace .. kHHeight");

// An HEVC sequence parameter set from its RBSP (the NAL without its two header bytes and emulation
// prevention) up to the bit depths: rb(i) is RBSP byte i < n.  false: an error
// (docs/INITSEGMENT.md lists them); every field of f is then 0.  Every loop is bounded by a
// constant of the syntax, so any bytes terminate.
template <class RB>
HLSP2P_RULE bool hevc_sps_parse(RB rb, int64_t n, HevcSpsFields& f) {
  f = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  SpsBits<RB> r = {rb, 8 * n, 0, false};
  r.u(4);  // sps_video_parameter_set_id
  const uint32_t L = r.u(3);  // sps_max_sub_layers_minus1
  const uint32_t nested = r.u(1);
  if (r.err || L == 7) return false;
  // profile_tier_level(1, L)
  const uint32_t space = r.u(2), tier = r.u(1), profile = r.u(5);
  const uint32_t compat = r.u(32), constraint_hi = r.u(16), constraint_lo = r.u(32), level = r.u(8);
  uint32_t has_profile = 0, has_level = 0;  // bit i: sub-layer i
  for (uint32_t i = 0; i < L; ++i) {
    has_profile |= r.u(1) << i;
    has_level |= r.u(1) << i;
  }
  if (L > 0)
    for (uint32_t i = L; i < 8; ++i) r.u(2);  // reserved_zero_2bits
  for (uint32_t i = 0; i < L; ++i) {
    if ((has_profile >> i) & 1) {  // 88 bits of a sub-layer's profile
      r.u(32);
      r.u(32);
      r.u(24);
    }
    if ((has_level >> i) & 1) r.u(8);
  }
  const uint32_t sps_id = r.ue();
  if (r.err || sps_id > 15) return false;
  const uint32_t chroma = r.ue();
  if (r.err || chroma > 3) return false;
  if (chroma == 3) r.u(1);  // separate_colour_plane
  const int64_t W = r.ue(), H = r.ue();
  int64_t left = 0, right = 0, top = 0, bottom = 0;
  if (r.u(1)) {  // conformance_window
    left = r.ue();
    right = r.ue();
    top = r.ue();
    bottom = r.ue();
  }
  const uint32_t depth_luma = r.ue(), depth_chroma = r.ue();
  if (r.err || depth_luma > 8 || depth_chroma > 8) return false;
  const int64_t cx = chroma == 1 || chroma == 2 ? 2 : 1, cy = chroma == 1 ? 2 : 1;
  const int64_t width = W - cx * (left + right), height = H - cy * (top + bottom);
  if (width < 1 || width > 65535 || height < 1 || height > 65535) return false;
  f.profile_space = static_cast<int32_t>(space);
  f.tier_flag = static_cast<int32_t>(tier);
  f.profile_idc = static_cast<int32_t>(profile);
  f.profile_compat = static_cast<int32_t>(compat);
  f.constraint_hi = static_cast<int32_t>(constraint_hi);
  f.constraint_lo = static_cast<int32_t>(constraint_lo);
  f.level_idc = static_cast<int32_t>(level);
  f.num_temporal_layers = static_cast<int32_t>(L + 1);
  f.temporal_id_nested = static_cast<int32_t>(nested);
  f.chroma_format_idc = static_cast<int32_t>(chroma);
  f.bit_depth_luma = static_cast<int32_t>(8 + depth_luma);
  f.bit_depth_chroma = static_cast<int32_t>(8 + depth_chroma);
  f.width = static_cast<int32_t>(width);
  f.height = static_cast<int32_t>(height);
  return true;
}

// x - y as a sample duration (unsigned == true: 0 .. 2^31 - 1) or composition offset (the int32
// range), exact for any int64 pair; fits == false: the caller stores 0 and flags bad_timestamps
struct Delta32 { int32_t v; bool fits; };
HLSP2P_RULE Delta32 delta32(int64_t x, int64_t y, bool non_negative) {
  const uint64_t ux = static_cast<uint64_t>(x), uy = static_cast<uint64_t>(y);
  if (x >= y) {
    const uint64_t d = ux - uy;
    return d <= 0x7fffffffu ? Delta32{static_cast<int32_t>(d), true} : Delta32{0, false};
  }
  const uint64_t d = uy - ux;
  if (non_negative || d > 0x80000000u) return {0, false};
  return {static_cast<int32_t>(-static_cast<int64_t>(d)), true};
}

// ---- moof boxes in front of the two mdat boxes (docs/FRAGMENT.md)
// A 90 kHz stamp x relative to `base`; with a reference time ref >= 0 the result is moved by the
// multiple of 2^33 that brings it within 2^32 of ref (hls.js's _PTSNormalize): the division
// floors.  Two's complement throughout, so stamps no demuxer writes wrap and never trap.
HLSP2P_RULE int64_t time_rel(int64_t x, int64_t base, int64_t ref) {
  uint64_t rel = static_cast<uint64_t>(x) - static_cast<uint64_t>(base);
  if (ref >= 0) {
    const int64_t t = static_cast<int64_t>(static_cast<uint64_t>(ref) - rel + (uint64_t(1) << 32));
    rel += static_cast<uint64_t>(t >> 33) << 33;  // an arithmetic shift: floor(t / 2^33)
  }
  return static_cast<int64_t>(rel);
}
// A 90 kHz time t >= 0 in units of the audio sample rate, rounded to nearest (exact while t * rate < 2^64 - 45000)
HLSP2P_RULE int64_t audio_rescale(int64_t t90k, int64_t rate) {
  return static_cast<int64_t>((static_cast<uint64_t>(t90k) * static_cast<uint64_t>(rate) + 45000u) / 90000u);
}

// What a segment's two tfdt boxes and its finfo row say about time: m clamped video samples with
// first stamp vdts, first audio stamp apts (< 0: no audio PES), the index's sample rate.
struct FragTimes { int64_t status, base, video_tfdt, audio_tfdt; };
HLSP2P_RULE FragTimes frag_times(int64_t m, int64_t vdts, int64_t apts, int64_t rate, int64_t time_base, int64_t time_ref,
                                 bool anchor) {
  const bool has_v = m > 0, has_a = apts >= 0;
  FragTimes f = {0, time_base, 0, 0};
  if (anchor) {
    const int64_t first = has_v && has_a ? (vdts < apts ? vdts : apts) : has_v ? vdts : apts;
    f.base = has_v || has_a ? static_cast<int64_t>(static_cast<uint64_t>(first) - static_cast<uint64_t>(time_ref)) : 0;
  }
  if (has_v) {
    const int64_t r = time_rel(vdts, f.base, time_ref);
    if (r < 0) f.status |= kTimeClamped;
    f.video_tfdt = r < 0 ? 0 : r;
  }
  if (has_a) {
    const int64_t r = time_rel(apts, f.base, time_ref);
    if (r < 0) f.status |= kTimeClamped;
    if (rate <= 0) f.status |= kNoRate;
    else f.audio_tfdt = audio_rescale(r < 0 ? 0 : r, rate);
  }
  return f;
}

// What the audio traf takes from the segment: the index's sample rate and the AAC frame, or, with a
// mpainfo row (docs/MPEGAUDIO.md) that has a config (frame_samples > 0), that row's rate and frame
struct FragAudio { int64_t rate; uint32_t duration; };
HLSP2P_RULE FragAudio frag_audio(int64_t sinfo_rate, const int64_t* mpainfo_row) {
  if (mpainfo_row && mpainfo_row[kMpFrameSamples] > 0)
    return {mpainfo_row[kMpSampleRate], static_cast<uint32_t>(mpainfo_row[kMpFrameSamples])};
  return {sinfo_rate, static_cast<uint32_t>(kAacFrameSamples)};
}

// The audio box offset a fragment trusts: rinfo's, brought to a multiple of 16 that leaves the
// gap in front of it and the box header behind it inside the region (>= audio_gap + 32 bytes)
HLSP2P_RULE int64_t frag_audio_box(int64_t a0, int64_t region, int64_t audio_gap) {
  return clamp(a0 & ~int64_t(15), audio_gap + 16, (region - 8) & ~int64_t(15));
}

// Dword i of the 22 in front of the video trun's entries, and of the 24 in front of the audio
// trun's, as numbers: the boxes hold them big-endian.  m / n entries, mfhd sequence number seq.
HLSP2P_RULE uint32_t moof_video_word(int i, uint32_t m, uint32_t seq, uint64_t tfdt) {
  const uint32_t size = kMoofVideoHead + kMoofVideoEntry * m;
  switch (i) {
    case 0: return size;
    case 1: return 0x6d6f6f66u;  // 'moof'
    case 2: return 16;
    case 3: return 0x6d666864u;  // 'mfhd'
    case 5: return seq;
    case 6: return size - 24;
    case 7: return 0x74726166u;  // 'traf'
    case 8: return 16;
    case 9: return 0x74666864u;  // 'tfhd'
    case 10: return 0x00020000u;  // default-base-is-moof
    case 11: return 1;            // track
    case 12: return 20;
    case 13: return 0x74666474u;  // 'tfdt'
    case 14: return 0x01000000u;  // version 1
    case 15: return static_cast<uint32_t>(tfdt >> 32);
    case 16: return static_cast<uint32_t>(tfdt);
    case 17: return size - 68;
    case 18: return 0x7472756eu;  // 'trun'
    case 19: return 0x01000f01u;  // version 1: data offset, duration, size, flags, signed cts
    case 20: return m;
    case 21: return size + 8;     // data_offset: behind the header of the mdat that follows
    default: return 0;
  }
}
// duration: the samples of one frame, the tfhd default (1,024 for AAC; docs/MPEGAUDIO.md for MPEG audio)
HLSP2P_RULE uint32_t moof_audio_word(int i, uint32_t n, uint32_t seq, uint64_t tfdt, uint32_t duration = kAacFrameSamples) {
  const uint32_t size = kMoofAudioHead + kMoofAudioEntry * n;
  switch (i) {
    case 0: return size;
    case 1: return 0x6d6f6f66u;
    case 2: return 16;
    case 3: return 0x6d666864u;
    case 5: return seq;
    case 6: return size - 24;
    case 7: return 0x74726166u;
    case 8: return 24;
    case 9: return 0x74666864u;
    case 10: return 0x00020028u;  // default-base-is-moof, default duration, default flags
    case 11: return 2;            // track
    case 12: return duration;     // samples of a frame
    case 13: return 0x02000000u;  // every frame is a sync sample
    case 14: return 20;
    case 15: return 0x74666474u;
    case 16: return 0x01000000u;
    case 17: return static_cast<uint32_t>(tfdt >> 32);
    case 18: return static_cast<uint32_t>(tfdt);
    case 19: return size - 76;
    case 20: return 0x7472756eu;
    case 21: return 0x00000201u;  // version 0: data offset, size
    case 22: return n;
    case 23: return size + 8;
    default: return 0;
  }
}

// ---- CEA-608/708 caption data in SEI NAL units (docs/CAPTIONS.md)
// header bytes of a NAL unit in front of its RBSP
HLSP2P_RULE int nal_header_bytes(bool hevc) { return hevc ? kHevcNalHeader : 1; }
// NAL row of a video ES with m access units: an SEI (H.264) or a prefix SEI (HEVC) of an access
// unit, with more clamped bytes than its header, is unescaped and walked.
HLSP2P_RULE bool cc_nal_candidate(bool hevc, int type, int64_t au, int64_t m, int64_t n) {
  return type == (hevc ? kSeiHevcPrefix : kSeiH264) && au >= 0 && au < m && n > nal_header_bytes(hevc);
}
// One sei_message header at p of the u unescaped bytes ub(0 .. u), u - p >= 2: payloadType T and
// payloadSize S with their FF extension bytes; p moves behind the header.  false: the header or
// the S payload bytes behind it run off the bytes, the walk ends.
template <class UB>
HLSP2P_RULE bool cc_message_header(UB ub, int u, int& p, int& T, int& S) {
  T = 0;
  while (p < u && ub(p) == 0xFF) {
    T += 255;
    ++p;
  }
  if (p >= u) return false;
  T += ub(p++);
  S = 0;
  while (p < u && ub(p) == 0xFF) {
    S += 255;
    ++p;
  }
  if (p >= u) return false;
  S += ub(p++);
  return S <= u - p;
}
// cc_count of the ATSC A/53 caption payload a message (T, S) at p holds, -1 for any other message:
// itu_t_t35 country 0xB5, provider 0x0031, 'GA94', user_data_type_code 3, and 10 + 3 cc_count <= S.
template <class UB>
HLSP2P_RULE int cc_ga94_match(UB ub, int p, int T, int S) {
  if (T != kSeiUserDataT35 || S < kCcHeadBytes + 2) return -1;
  if (ub(p) != 0xB5 || ub(p + 1) != 0x00 || ub(p + 2) != 0x31 || ub(p + 3) != 'G' || ub(p + 4) != 'A' ||
      ub(p + 5) != '9' || ub(p + 6) != '4' || ub(p + 7) != 3)
    return -1;
  const int c = ub(p + kCcHeadBytes) & kCcMaxTriples;
  return kCcHeadBytes + 2 + 3 * c <= S ? c : -1;
}
// The first caption message of the u unescaped bytes of an SEI: its sample is
// ub(at .. at + 2 + 3 count).  count < 0: none.  Every step consumes at least two bytes.
struct CcMatch { int at, count; };
template <class UB>
HLSP2P_RULE CcMatch cc_find(UB ub, int u) {
  int p = 0;
  while (u - p >= 2) {
    int T, S;
    if (!cc_message_header(ub, u, p, T, S)) break;
    const int c = cc_ga94_match(ub, p, T, S);
    if (c >= 0) return {p + kCcHeadBytes, c};
    p += S;
  }
  return {0, -1};
}
// Triple (f, b1, b2) of a sample gives a 608 byte pair to field 0 or 1, or to none (-1): cc_valid
// set, cc_type 0 or 1, and the two bytes without their parity bits not both zero.
HLSP2P_RULE int cc_608_field(int f, int b1, int b2) {
  return (f & 4) && (f & 3) < 2 && ((b1 | b2) & 0x7f) != 0 ? (f & 3) : -1;
}
// The status bits of a segment, from its demux and index rows alone.
HLSP2P_RULE int64_t cc_status(const Segment& s, const int64_t* sinfo) {
  int64_t st = 0;
  if (sinfo[kStatus] & kNalOverflow) st |= kCcTruncated;
  if (!video_supported(s.info[ts::kVideoType]) && clamp(s.info[ts::kVideoBytes], 0, s.cap) > 0) st |= kCcUnsupportedVideo;
  return st;
}
}  // namespace es

// ---------------------------------------------------------------- fragmented MP4 demux (docs/FMP4DEMUX.md)
// A reader `rd` gives rd.u8(p), byte p of the segment, and rd.be32(p), and is asked only for bytes of [0, n).  Offsets are
// int64 and wrap like two's complement where a file can make them overflow.
namespace mp4 {
constexpr uint32_t fourcc(char a, char b, char c, char d) {
  return (uint32_t(uint8_t(a)) << 24) | (uint32_t(uint8_t(b)) << 16) | (uint32_t(uint8_t(c)) << 8) | uint32_t(uint8_t(d));
}
constexpr uint32_t kMoof = fourcc('m', 'o', 'o', 'f'), kEmsg = fourcc('e', 'm', 's', 'g'), kMfhd = fourcc('m', 'f', 'h', 'd'),
                   kTraf = fourcc('t', 'r', 'a', 'f'), kTfhd = fourcc('t', 'f', 'h', 'd'), kTfdt = fourcc('t', 'f', 'd', 't'),
                   kTrun = fourcc('t', 'r', 'u', 'n');
HLSP2P_RULE int64_t wrap_add(int64_t a, int64_t b) {
  return static_cast<int64_t>(static_cast<uint64_t>(a) + static_cast<uint64_t>(b));
}
HLSP2P_RULE int64_t wrap_sub(int64_t a, int64_t b) {
  return static_cast<int64_t>(static_cast<uint64_t>(a) - static_cast<uint64_t>(b));
}
// big-endian fields: rd.be32(p) is the four bytes at p, for a reader that has a faster way than four u8
template <class R>
HLSP2P_RULE uint32_t be32_bytes(R& rd, int64_t p) {
  return (uint32_t(rd.u8(p)) << 24) | (uint32_t(rd.u8(p + 1)) << 16) | (uint32_t(rd.u8(p + 2)) << 8) | uint32_t(rd.u8(p + 3));
}
template <class R>
HLSP2P_RULE uint32_t be32(R& rd, int64_t p) { return rd.be32(p); }
template <class R>
HLSP2P_RULE uint64_t be64(R& rd, int64_t p) {
  return (uint64_t(be32(rd, p)) << 32) | be32(rd, p + 4);
}

// The box header at p of [p, limit).  !ok: no box there (fewer than 8 bytes, a 64-bit size of 2^31
// or more, a size below the header or beyond limit); type is set whenever 8 bytes were there.
struct Box {
  bool ok;
  uint32_t type;
  int64_t hdr, size;
};
template <class R>
HLSP2P_RULE Box box_at(R& rd, int64_t p, int64_t limit) {
  Box b = {false, 0, 8, 0};
  if (limit - p < 8) return b;
  const uint32_t size32 = be32(rd, p);
  b.type = be32(rd, p + 4);
  b.size = size32;
  if (size32 == 1) {
    if (limit - p < 16) return b;
    const uint64_t large = be64(rd, p + 8);
    if (large >= 0x80000000ull) return b;
    b.hdr = 16;
    b.size = static_cast<int64_t>(large);
  } else if (size32 == 0) {
    b.size = limit - p;
  }
  b.ok = b.size >= b.hdr && b.size <= limit - p;
  return b;
}

// The top level of a segment of n bytes: on_moof(k, p, box) / on_emsg(k, p, box) for the k-th of
// each, in order; every step consumes at least 8 bytes.
struct TopOut { int64_t status, n_moof, n_emsg; };
template <class R, class FM, class FE>
HLSP2P_RULE TopOut top_walk(R& rd, int64_t n, FM&& on_moof, FE&& on_emsg) {
  TopOut o = {0, 0, 0};
  int64_t p = 0;
  while (p < n) {
    const Box b = box_at(rd, p, n);
    if (!b.ok) {
      o.status |= kBadBox;
      break;
    }
    if (b.type == kMoof) on_moof(o.n_moof++, p, b);
    else if (b.type == kEmsg) on_emsg(o.n_emsg++, p, b);
    p += b.size;
  }
  return o;
}

// slot of track_ID id among a segment's kTracks configured tracks, -1: none
HLSP2P_RULE int track_slot(const int64_t* tracks, int64_t id) {
  for (int s = 0; s < kTracks; ++s)
    if (tracks[s * kTrackWords + kTkId] > 0 && tracks[s * kTrackWords + kTkId] == id) return s;
  return -1;
}
// the video track is indexed: a NAL-structured codec with a usable length size
HLSP2P_RULE bool video_indexed(const int64_t* tracks) {
  const int64_t L = tracks[kTkNalLengthSize];
  return tracks[kTkId] > 0 && es::video_supported(tracks[kTkCodecType]) && (L == 1 || L == 2 || L == 4);
}

// One trun of a configured track as moof_walk hands it on.
struct Run {
  int track;
  int64_t count, entries;  // whole entries that fit, and where the first one lies
  uint32_t flags;          // tr_flags | version << 24
  int64_t traf_run;        // 0: the first run of its traf
  uint32_t def_duration, def_size, def_flags;
  int64_t first_flags;  // -1: absent
  bool has_start;       // data_offset present, or the first run of its traf
  int64_t start;
  bool has_tfdt;  // of its traf
  int64_t tfdt;
};
struct MoofOut { int64_t status, seq, n_other, n_run; };
HLSP2P_RULE int run_stride(uint32_t flags) { return 4 * __builtin_popcount((flags >> 8) & 0xf); }

// The children of one traf, [p, tend) inside the moof at mp; on_other(type, p, box) for a child
// the demux does not read.
template <class R, class F, class G>
HLSP2P_RULE void traf_walk(R& rd, int64_t mp, int64_t p, int64_t tend, const int64_t* tracks, int64_t n, MoofOut& o,
                           F&& on_run, G&& on_other) {
  int slot = -2;  // -2: no usable tfhd so far, -1: a track that is not configured
  bool seen_tfhd = false, seen_tfdt = false, seen_trun = false, has_tfdt = false;
  int64_t tfdt = 0, base = mp, traf_run = 0;
  uint32_t def_duration = 0, def_size = 0, def_flags = 0;
  while (p < tend) {
    const Box b = box_at(rd, p, tend);
    if (!b.ok) {
      o.status |= kBadBox;
      break;
    }
    const int64_t body = p + b.hdr, bend = p + b.size, len = bend - body;
    if (b.type == kTfhd && !seen_tfhd) {
      seen_tfhd = true;
      const uint32_t f = len >= 8 ? be32(rd, body) & 0xffffffu : 0;
      const int64_t need = 8 + ((f & 1) ? 8 : 0) + ((f & 2) ? 4 : 0) + ((f & 8) ? 4 : 0) + ((f & 0x10) ? 4 : 0) +
                           ((f & 0x20) ? 4 : 0);
      if (len < need) {
        o.status |= kBadBox;
      } else {
        slot = track_slot(tracks, be32(rd, body + 4));
        int64_t q = body + 8;
        if (f & 1) {
          base = static_cast<int64_t>(be64(rd, q));
          q += 8;
        }
        if (f & 2) q += 4;
        if (slot >= 0) {
          const int64_t* t = tracks + slot * kTrackWords;
          def_duration = static_cast<uint32_t>(t[kTkDefDuration]);
          def_size = static_cast<uint32_t>(t[kTkDefSize]);
          def_flags = static_cast<uint32_t>(t[kTkDefFlags]);
        }
        if (f & 8) {
          def_duration = be32(rd, q);
          q += 4;
        }
        if (f & 0x10) {
          def_size = be32(rd, q);
          q += 4;
        }
        if (f & 0x20) def_flags = be32(rd, q);
      }
    } else if (b.type == kTfdt && !seen_tfdt && !seen_trun) {
      seen_tfdt = true;
      const int version = len >= 8 ? rd.u8(body) : 0;
      if (len < (version == 0 ? 8 : 12)) {
        o.status |= kBadBox;
      } else {
        tfdt = version == 0 ? static_cast<int64_t>(be32(rd, body + 4)) : static_cast<int64_t>(be64(rd, body + 4));
        has_tfdt = true;
      }
    } else if (b.type == kTrun) {
      seen_trun = true;
      if (slot == -2) {
        o.status |= kBadBox;
      } else if (slot >= 0) {
        const uint32_t vf = len >= 8 ? be32(rd, body) : 0;
        const uint32_t f = vf & 0xffffffu;
        if (len < 8 + ((f & 1) ? 4 : 0) + ((f & 4) ? 4 : 0)) {
          o.status |= kBadBox;
        } else {
          const uint32_t sample_count = be32(rd, body + 4);
          int64_t q = body + 8;
          Run r = {slot, 0, 0, vf, traf_run, def_duration, def_size, def_flags, -1, traf_run == 0, base, has_tfdt, tfdt};
          if (f & 1) {
            r.has_start = true;
            r.start = wrap_add(base, static_cast<int32_t>(be32(rd, q)));
            q += 4;
          }
          if (f & 4) {
            r.first_flags = be32(rd, q);
            q += 4;
          }
          const int stride = run_stride(f);
          const int64_t fit = stride ? (bend - q) / stride : n;
          r.count = sample_count < fit ? sample_count : fit;
          r.entries = q;
          if (r.count < sample_count) o.status |= kBadBox;
          on_run(o.n_run, r);
          ++o.n_run;
          ++traf_run;
        }
      }
    } else {
      on_other(b.type, p, b);
    }
    p = bend;
  }
  if (slot == -2) o.status |= kBadBox;
  else if (slot == -1) ++o.n_other;
  else if (!has_tfdt) o.status |= kNoTfdt;
}
template <class R, class F>
HLSP2P_RULE void traf_walk(R& rd, int64_t mp, int64_t p, int64_t tend, const int64_t* tracks, int64_t n, MoofOut& o,
                           F&& on_run) {
  traf_walk(rd, mp, p, tend, tracks, n, o, on_run, [](uint32_t, int64_t, const Box&) {});
}

// The children of the moof box b at mp: on_run(j, run) for the j-th trun of a configured track.
template <class R, class F>
HLSP2P_RULE MoofOut moof_walk(R& rd, int64_t mp, const Box& b, const int64_t* tracks, int64_t n, F&& on_run) {
  MoofOut o = {0, -1, 0, 0};
  bool seen_mfhd = false;
  const int64_t mend = mp + b.size;
  int64_t p = mp + b.hdr;
  while (p < mend) {
    const Box c = box_at(rd, p, mend);
    if (!c.ok) {
      o.status |= kBadBox;
      break;
    }
    const int64_t body = p + c.hdr, bend = p + c.size;
    if (c.type == kMfhd && !seen_mfhd) {
      seen_mfhd = true;
      if (bend - body >= 8) o.seq = be32(rd, body + 4);
      else o.status |= kBadBox;
    } else if (c.type == kTraf) {
      traf_walk(rd, mp, body, bend, tracks, n, o, on_run);
    }
    p = bend;
  }
  return o;
}

// Sample j of a run: each field from its entry, else the run's default.
struct Sample {
  uint32_t size, duration, flags;
  int32_t cts;
};
template <class R>
HLSP2P_RULE Sample sample_at(R& rd, int64_t entries, uint32_t flags, int64_t j, uint32_t def_duration, uint32_t def_size,
                             uint32_t def_flags, int64_t first_flags) {
  Sample s = {def_size, def_duration, def_flags, 0};
  int64_t q = entries + j * run_stride(flags);
  if (flags & 0x100) {
    s.duration = be32(rd, q);
    q += 4;
  }
  if (flags & 0x200) {
    s.size = be32(rd, q);
    q += 4;
  }
  if (flags & 0x400) {
    s.flags = be32(rd, q);
    q += 4;
  }
  if (flags & 0x800) s.cts = static_cast<int32_t>(be32(rd, q));  // signed in both versions
  if (j == 0 && first_flags >= 0) s.flags = static_cast<uint32_t>(first_flags);
  return s;
}
// [off, off + size) clamped to the segment's [0, n)
struct Placed {
  int64_t off, size;
  bool clipped;
};
HLSP2P_RULE Placed place_sample(int64_t off, uint32_t size, int64_t n) {
  const int64_t end = wrap_add(off, size);
  const bool inside = off >= 0 && end >= off && end <= n;
  const int64_t a = clamp(off, 0, n);
  const int64_t e = end < off ? n : clamp(end, a, n);
  return {a, e - a, !inside};
}

// One step of the length-prefixed walk at q of a sample that ends at `end`: 1: the NAL (s, len);
// 0: no length field fits any more (clean iff q == end); 2: a length beyond the sample.
template <class R>
HLSP2P_RULE int nal_step(R& rd, int64_t q, int64_t end, int L, int64_t& s, int64_t& len) {
  if (q + L > end) return 0;
  uint32_t v = 0;
  for (int i = 0; i < L; ++i) v = (v << 8) | uint32_t(rd.u8(q + i));
  s = q + L;
  if (v > end - s) return 2;
  len = v;
  return 1;
}

// 'https://aomedia.org/emsg/ID3', four characters per word
constexpr int kId3SchemeChars = 28;
HLSP2P_RULE uint32_t id3_scheme_word(int w) {
  switch (w) {
    case 0: return fourcc('h', 't', 't', 'p'); case 1: return fourcc('s', ':', '/', '/');
    case 2: return fourcc('a', 'o', 'm', 'e'); case 3: return fourcc('d', 'i', 'a', '.');
    case 4: return fourcc('o', 'r', 'g', '/'); case 5: return fourcc('e', 'm', 's', 'g');
    case 6: return fourcc('/', 'I', 'D', '3'); default: return 0;
  }
}
// The zero-terminated string at q of [.., bend): the position behind its terminator, -1 when it
// does not end inside; id3: it is the ID3 scheme, terminator included.
template <class R>
HLSP2P_RULE int64_t emsg_string(R& rd, int64_t q, int64_t bend, bool& id3) {
  bool match = true;
  for (int i = 0; q < bend; ++q, ++i) {
    const uint32_t c = rd.u8(q);
    if (c == 0) {
      id3 = match && i == kId3SchemeChars;
      return q + 1;
    }
    match = match && i < kId3SchemeChars && c == ((id3_scheme_word(i >> 2) >> (24 - 8 * (i & 3))) & 0xff);
    if (i >= kId3SchemeChars) i = kId3SchemeChars;  // stays behind the scheme, never overflows
  }
  return -1;
}
struct Emsg {
  bool ok;
  int64_t version, timescale, time, is_delta, duration, id, data_off, data_len, is_id3;
};
template <class R>
HLSP2P_RULE Emsg emsg_parse(R& rd, int64_t p, const Box& b) {
  Emsg e = {false, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  const int64_t body = p + b.hdr, bend = p + b.size;
  if (bend - body < 4) return e;
  e.version = rd.u8(body);
  bool id3 = false, other = false;
  int64_t q;
  if (e.version == 0) {
    q = emsg_string(rd, body + 4, bend, id3);
    if (q >= 0) q = emsg_string(rd, q, bend, other);
    if (q < 0 || bend - q < 16) return e;
    e.timescale = be32(rd, q);
    e.time = be32(rd, q + 4);
    e.is_delta = 1;
    e.duration = be32(rd, q + 8);
    e.id = be32(rd, q + 12);
    q += 16;
  } else if (e.version == 1) {
    if (bend - body < 24) return e;
    e.timescale = be32(rd, body + 4);
    e.time = static_cast<int64_t>(be64(rd, body + 8));
    e.duration = be32(rd, body + 16);
    e.id = be32(rd, body + 20);
    q = emsg_string(rd, body + 24, bend, id3);
    if (q >= 0) q = emsg_string(rd, q, bend, other);
    if (q < 0) return e;
  } else {
    return e;
  }
  e.data_off = q;
  e.data_len = bend - q;
  e.is_id3 = id3 ? 1 : 0;
  e.ok = true;
  return e;
}

// What the sample pass settles of a run beyond the box walk: where its bytes and its clock start.
// `run(k)` is recorded run k <= r as a Run.  The start comes from the nearest run of the same traf
// that has one of its own (the first run of a traf always has); the time from the nearest first run
// of a traf of the same track that has a tfdt, else 0 at the track's sample 0.
template <class A>
HLSP2P_RULE int64_t start_anchor(A&& run, int64_t r) {
  while (!run(r).has_start) --r;
  return r;
}
template <class A>
HLSP2P_RULE int64_t time_anchor(A&& run, int64_t r) {
  const int track = run(r).track;
  for (; r >= 0; --r) {
    const Run k = run(r);
    if (k.track == track && k.traf_run == 0 && k.has_tfdt) return r;
  }
  return -1;
}
// A duration as msamples holds it: fits == false stores 0 and flags bad_timestamps
HLSP2P_RULE es::Delta32 duration32(uint32_t d) {
  return d <= 0x7fffffffu ? es::Delta32{static_cast<int32_t>(d), true} : es::Delta32{0, false};
}

// ---------------------------------------------------------------- cbcs decryption (docs/CBCS.md)
constexpr uint32_t kSenc = fourcc('s', 'e', 'n', 'c');
// Per_Sample_IV_Size / constant_IV_size as the walk uses it: 8 or 16, anything else is 0
HLSP2P_RULE int iv_bytes(int64_t v) { return v == 8 || v == 16 ? static_cast<int>(v) : 0; }

// The trafs of the moof box b at mp that have a trun of a configured track: on_traf(slot, j0,
// runs, sp, senc) with the track slot, the traf's runs [j0, j0 + runs) among the moof's (the j of
// moof_walk) and its first senc child at sp (sp < 0: none), wherever it stands among the children.
template <class R, class F>
HLSP2P_RULE void senc_walk(R& rd, int64_t mp, const Box& b, const int64_t* tracks, int64_t n, F&& on_traf) {
  MoofOut o = {0, -1, 0, 0};
  const int64_t mend = mp + b.size;
  int64_t p = mp + b.hdr;
  while (p < mend) {
    const Box c = box_at(rd, p, mend);
    if (!c.ok) break;
    if (c.type == kTraf) {
      const int64_t j0 = o.n_run;
      int slot = -1;
      int64_t sp = -1;
      Box senc = {false, 0, 8, 0};
      traf_walk(rd, mp, p + c.hdr, p + c.size, tracks, n, o, [&](int64_t, const Run& r) { slot = r.track; },
                [&](uint32_t type, int64_t q, const Box& k) {
                  if (type == kSenc && sp < 0) {
                    sp = q;
                    senc = k;
                  }
                });
      if (o.n_run > j0) on_traf(slot, j0, o.n_run - j0, sp, senc);
    }
    p += c.size;
  }
}

// The fixed fields of the senc box b at sp.  !ok: the body is too short for them.
struct SencHead {
  bool ok;
  uint32_t flags;
  int64_t count, at, end;  // sample_count, the first entry, the box end
};
template <class R>
HLSP2P_RULE SencHead senc_head(R& rd, int64_t sp, const Box& b) {
  const int64_t body = sp + b.hdr, bend = sp + b.size;
  if (bend - body < 8) return {false, 0, 0, body, bend};
  return {true, be32(rd, body) & 0xffffffu, static_cast<int64_t>(be32(rd, body + 4)), body + 8, bend};
}
template <class R>
HLSP2P_RULE int64_t be16(R& rd, int64_t p) { return (int64_t(rd.u8(p)) << 8) | rd.u8(p + 1); }
// The entry at q of a senc that ends at bend: the position behind it, -1 when the box end cuts
// it; nsub is its subsample_count, -1 when the box has no subsample tables.
template <class R>
HLSP2P_RULE int64_t senc_entry(R& rd, int64_t q, int64_t bend, int iv_size, bool subs, int64_t& nsub) {
  nsub = -1;
  if (bend - q < iv_size) return -1;
  int64_t e = q + iv_size;
  if (subs) {
    if (bend - e < 2) return -1;
    nsub = be16(rd, e);
    e += 2;
    if (bend - e < 6 * nsub) return -1;
    e += 6 * nsub;
  }
  return e;
}
// The protected ranges of the sample at o of z bytes, in order: on_range(offset, length).  sub is
// where its nsub (clear u16, protected u32) pairs lie; nsub < 0: the sample is one range.  false: a
// sum runs beyond the sample (bad_senc); the ranges in front of it have been handed on.
template <class R, class F>
HLSP2P_RULE bool sample_ranges(R& rd, int64_t o, int64_t z, int64_t sub, int64_t nsub, F&& on_range) {
  if (nsub < 0) {
    on_range(o, z);
    return true;
  }
  int64_t q = 0;
  for (int64_t i = 0; i < nsub; ++i) {
    const int64_t clear = be16(rd, sub + 6 * i), prot = be32(rd, sub + 6 * i + 2);
    if (clear > z - q) return false;
    q += clear;
    if (prot > z - q) return false;
    on_range(o + q, prot);
    q += prot;
  }
  return true;
}
// The cipher blocks of a range of P bytes under the pattern crypt:skip (skip 0: every block), and
// where block j lies.  A trailing partial crypt group stays clear; a block that ends with the
// range is encrypted.
HLSP2P_RULE int64_t cipher_blocks(int64_t P, int64_t c, int64_t s) {
  const int64_t nb = P / 16;
  if (c <= 0 || s <= 0) return nb;
  return (nb / (c + s)) * c + (nb % (c + s) >= c ? c : 0);
}
HLSP2P_RULE int64_t cipher_block_at(int64_t j, int64_t c, int64_t s) {
  if (c <= 0 || s <= 0) return 16 * j;
  return 16 * ((j / c) * (c + s) + j % c);
}
// two byte spans [a0, a1) and [b0, b1), neither empty, share a byte
HLSP2P_RULE bool spans_meet(int64_t a0, int64_t a1, int64_t b0, int64_t b1) {
  return a0 < a1 && b0 < b1 && a0 < b1 && b0 < a1;
}

// ---------------------------------------------------------------- cenc decryption (docs/CENC.md)
// The protected bytes of a sample form one AES-CTR keystream that runs on across its clear bytes.
// A range of len >= 1 bytes whose first byte is byte p0 of that stream is cut into units, one per
// keystream block it touches.
HLSP2P_RULE int64_t ctr_units(int64_t p0, int64_t len) { return len > 0 ? (p0 + len + 15) / 16 - p0 / 16 : 0; }
// keystream block of unit m
HLSP2P_RULE int64_t ctr_unit_block(int64_t p0, int64_t m) { return p0 / 16 + m; }
// where byte 0 of keystream block j would lie in the segment for a range at off (below off for
// the block a range starts inside)
HLSP2P_RULE int64_t ctr_block_at(int64_t off, int64_t p0, int64_t j) { return off + 16 * j - p0; }
// Counter block j of a 16-byte IV held as four little-endian words (as loaded): the last 8 bytes
// are a big-endian integer that j is added to modulo 2^64; the first 8 never change.
HLSP2P_RULE uint32_t ctr_bswap(uint32_t v) {
  return (v << 24) | ((v & 0xff00u) << 8) | ((v >> 8) & 0xff00u) | (v >> 24);
}
HLSP2P_RULE void ctr_block(const uint32_t iv[4], int64_t j, uint32_t out[4]) {
  const uint64_t low = ((static_cast<uint64_t>(ctr_bswap(iv[2])) << 32) | ctr_bswap(iv[3])) + static_cast<uint64_t>(j);
  out[0] = iv[0];
  out[1] = iv[1];
  out[2] = ctr_bswap(static_cast<uint32_t>(low >> 32));
  out[3] = ctr_bswap(static_cast<uint32_t>(low));
}
}  // namespace mp4

// ---------------------------------------------------------------- packed audio (docs/PACKEDAUDIO.md)
// One or more ID3v2 tags in front of raw ADTS frames.  A reader `rd` is the one of namespace mp4:
// rd.u8(p) and rd.be32(p) of the segment, asked only for bytes of [0, n).
namespace es {
// 'com.apple.streaming.transportStreamTimestamp', four characters per word; a NUL and the 8-byte stamp follow
constexpr int kPackedOwnerWords = 11;
constexpr int kPackedPrivBytes = 4 * kPackedOwnerWords + 1 + 8;
HLSP2P_RULE uint32_t packed_owner_word(int w) {
  using mp4::fourcc;
  switch (w) {
    case 0: return fourcc('c', 'o', 'm', '.'); case 1: return fourcc('a', 'p', 'p', 'l');
    case 2: return fourcc('e', '.', 's', 't'); case 3: return fourcc('r', 'e', 'a', 'm');
    case 4: return fourcc('i', 'n', 'g', '.'); case 5: return fourcc('t', 'r', 'a', 'n');
    case 6: return fourcc('s', 'p', 'o', 'r'); case 7: return fourcc('t', 'S', 't', 'r');
    case 8: return fourcc('e', 'a', 'm', 'T'); case 9: return fourcc('i', 'm', 'e', 's');
    case 10: return fourcc('t', 'a', 'm', 'p'); default: return 0;
  }
}
HLSP2P_RULE bool syncsafe_ok(uint32_t v) { return (v & 0x80808080u) == 0; }
HLSP2P_RULE int64_t syncsafe28(uint32_t v) {
  return (int64_t((v >> 24) & 0x7f) << 21) | (int64_t((v >> 16) & 0x7f) << 14) | (int64_t((v >> 8) & 0x7f) << 7) |
         int64_t(v & 0x7f);
}

// The ID3v2 tag header at t of [.., n).  !ok: no tag there.
struct Id3Tag {
  bool ok;
  int version, flags;
  int64_t size, total;  // the frames' bytes, and the whole tag with header and footer
};
template <class R>
HLSP2P_RULE Id3Tag id3_tag_at(R& rd, int64_t t, int64_t n) {
  Id3Tag g = {false, 0, 0, 0, 0};
  if (t + 10 > n) return g;
  const uint32_t head = mp4::be32(rd, t);
  if ((head >> 8) != 0x494433u) return g;  // 'ID3'
  g.version = static_cast<int>(head & 0xff);
  if (g.version == 0xff || rd.u8(t + 4) == 0xff) return g;
  g.flags = rd.u8(t + 5);
  const uint32_t s = mp4::be32(rd, t + 6);
  if (!syncsafe_ok(s)) return g;
  g.size = syncsafe28(s);
  g.total = 10 + g.size + ((g.flags & 0x10) ? 10 : 0);
  g.ok = true;
  return g;
}
// The 33-bit stamp of the first PRIV frame of the tag at t that carries one, -1: none.
template <class R>
HLSP2P_RULE int64_t id3_timestamp(R& rd, int64_t t, const Id3Tag& g) {
  if ((g.version != 3 && g.version != 4) || (g.flags & 0xC0)) return -1;
  int64_t f = t + 10;
  const int64_t end = f + g.size;
  for (int i = 0; i < kPackedMaxId3Frames && f + 10 <= end && rd.u8(f) != 0; ++i) {
    const uint32_t raw = mp4::be32(rd, f + 4);
    if (g.version == 4 && !syncsafe_ok(raw)) break;
    const int64_t fsize = g.version == 4 ? syncsafe28(raw) : int64_t(raw);
    if (fsize > end - (f + 10)) break;
    if (fsize == kPackedPrivBytes && mp4::be32(rd, f) == mp4::fourcc('P', 'R', 'I', 'V')) {
      const int64_t body = f + 10;
      bool match = rd.u8(body + 4 * kPackedOwnerWords) == 0;
      for (int w = 0; w < kPackedOwnerWords; ++w) match = match && mp4::be32(rd, body + 4 * w) == packed_owner_word(w);
      if (match) {
        const int64_t v = body + 4 * kPackedOwnerWords + 1;
        return (int64_t(mp4::be32(rd, v) & 1u) << 32) | int64_t(mp4::be32(rd, v + 4));
      }
    }
    f += 10 + fsize;
  }
  return -1;
}
// The leading tags: T is where the audio starts, or the tag that passes the end (kPaBadId3).
struct PackedTags { int64_t status, T, n_tags, ts; };
template <class R>
HLSP2P_RULE PackedTags packed_tags(R& rd, int64_t n) {
  PackedTags r = {0, 0, 0, -1};
  for (int i = 0; i < kPackedMaxTags; ++i) {
    const Id3Tag g = id3_tag_at(rd, r.T, n);
    if (!g.ok) break;
    if (r.T + g.total > n) {
      r.status |= kPaBadId3;
      break;
    }
    if (r.ts < 0) r.ts = id3_timestamp(rd, r.T, g);
    r.T += g.total;
    ++r.n_tags;
  }
  if (r.ts < 0) r.status |= kPaNoTimestamp;
  return r;
}

// What the tags and the frame walk leave of a segment of n bytes; the three info rows are made of it.
struct PackedSummary { int64_t status, T, n_tags, ts, n_frames, stop, rate, chans, n; };
HLSP2P_RULE int64_t packed_groups(int64_t n_frames) { return (n_frames + kPackedFramesPerPes - 1) / kPackedFramesPerPes; }
// the stamp of group k: not wrapped at 2^33
HLSP2P_RULE int64_t packed_stamp(int64_t ts, int64_t k, int64_t rate) {
  return rate > 0 ? ts + (k * kPackedFramesPerPes * kAacFrameSamples * 90000 + rate / 2) / rate : ts;
}
// rate_index / channel byte pair of the first frame: A[q + 2], A[q + 3]
HLSP2P_RULE int adts_channels(int b2, int b3) { return ((b2 & 1) << 2) | (b3 >> 6); }
HLSP2P_RULE PackedSummary packed_summary(const PackedTags& g, int64_t n_frames, int64_t stop, int64_t rate, int64_t chans,
                                         int64_t n, int64_t max_pes) {
  PackedSummary s = {g.status, g.T, g.n_tags, g.ts, n_frames, stop, rate, chans, n};
  if (!(g.status & kPaBadId3)) {
    if (n_frames == 0) s.status |= kPaNoFrame;
    else if (stop != n) s.status |= kPaTrailingBytes;
    if (n_frames > 0 && rate == 0) s.status |= kPaBadRate;
  }
  if (packed_groups(n_frames) > max_pes) s.status |= kPaPesOverflow;
  return s;
}
HLSP2P_RULE int64_t packed_info_word(int i, const PackedSummary& s, int64_t max_pes) {
  const int64_t groups = packed_groups(s.n_frames), rec = groups < max_pes ? groups : max_pes;
  switch (i) {
    case ts::kStatus: return groups > max_pes ? int64_t(ts::kPesOverflow) : 0;
    case ts::kPmtPid: case ts::kVideoPid: case ts::kAudioPid: case ts::kId3Pid: return -1;
    case ts::kAudioBytes: return s.n - s.T;
    case ts::kId3Bytes: return s.T;
    case ts::kNumAudioPes: return groups;
    case ts::kNumId3Pes: return s.T > 0;
    case ts::kAudioType: return ts::kAdtsAac;
    case ts::kPayloadBytes: return s.n;
    case ts::kFirstPts: case ts::kLastPts: return -1;
    case ts::kFirstPts + 1: return rec > 0 ? packed_stamp(s.ts, 0, s.rate) : -1;
    case ts::kLastPts + 1: return rec > 0 ? packed_stamp(s.ts, rec - 1, s.rate) : -1;
    case ts::kFirstPts + 2: case ts::kLastPts + 2: return s.T > 0 ? s.ts : -1;
    case ts::kAudioEsOffset: return s.T;
    default: return 0;  // no packets, no video, the id3 ES at 0
  }
}
HLSP2P_RULE int64_t packed_sinfo_word(int i, const PackedSummary& s) {
  switch (i) {
    case kStatus: return (s.status & kPaTrailingBytes) ? int64_t(kAdtsError) : 0;
    case kFirstKeyframeAu: return -1;
    case kNumAdtsFrames: return s.n_frames;
    case kAudioSampleRate: return s.rate;
    case kAudioChannels: return s.chans;
    default: return 0;
  }
}
HLSP2P_RULE int64_t packed_painfo_word(int i, const PackedSummary& s) {
  switch (i) {
    case kPaStatus: return s.status;
    case kPaId3Bytes: return s.T;
    case kPaNumTags: return s.n_tags;
    case kPaTimestamp: return s.ts;
    case kPaNumFrames: return s.n_frames;
    case kPaStopOffset: return s.stop;
    case kPaSampleRate: return s.rate;
    default: return s.chans;
  }
}
}  // namespace es
}  // namespace hlsp2p
