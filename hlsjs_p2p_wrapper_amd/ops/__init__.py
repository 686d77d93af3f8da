"""Batched segment ops (``aes``, ``crc``, ``segment``, ``tsdemux``, ``esindex``, ``remux``, ``fragment``,
``codecconfig``, ``hevcconfig``, ``sampleaes``, ``captions``, ``mp4demux``, ``cbcs``, ``cenc``, ``packedaudio``,
``mpegaudio``, ``ac3audio``):
import the
submodule you need.  The entry points of the sample index, of the remux, of the two codec configurations, of the
SAMPLE-AES decrypt, of the caption extraction, of the fragmented-MP4 demux, of the cbcs and cenc decrypts and of
the packed-audio demux and of the MPEG audio and AC-3 / E-AC-3 remuxes are
also reachable from the package
(``ops.index_batch``,
``ops.EsIndex``, ``ops.remux_batch``,
``ops.Remuxed``, ``ops.fragment_batch``, ``ops.Fragments``,
``ops.config_batch``, ``ops.CodecConfig``, ``ops.hevc_config_batch``,
``ops.HevcConfig``, ``ops.sample_decrypt_batch``, ``ops.SampleAes``, ``ops.caption_batch``,
``ops.Captions``, ``ops.mp4_demux_batch``, ``ops.Mp4Demux``, ``ops.Mp4Track``, ``ops.cbcs_decrypt_batch``,
``ops.Cbcs``, ``ops.Mp4Protection``, ``ops.cenc_decrypt_batch``, ``ops.Cenc``,
``ops.packed_audio_batch``, ``ops.PackedAudio``, ``ops.mpeg_audio_batch``, ``ops.MpegAudio``,
``ops.ac3_audio_batch``, ``ops.Ac3Audio``), resolved on first use."""

_ESINDEX = ("index_batch", "EsIndex")
_REMUX = ("remux_batch", "Remuxed")
_FRAGMENT = ("fragment_batch", "Fragments")
_CODECCONFIG = ("config_batch", "CodecConfig")
_HEVCCONFIG = ("hevc_config_batch", "HevcConfig")
_SAMPLEAES = ("sample_decrypt_batch", "SampleAes")
_CAPTIONS = ("caption_batch", "Captions")
_MP4DEMUX = ("mp4_demux_batch", "Mp4Demux", "Mp4Track")
_CBCS = ("cbcs_decrypt_batch", "Cbcs", "Mp4Protection")
_CENC = ("cenc_decrypt_batch", "Cenc")
_PACKEDAUDIO = ("packed_audio_batch", "PackedAudio")
_MPEGAUDIO = ("mpeg_audio_batch", "MpegAudio")
_AC3AUDIO = ("ac3_audio_batch", "Ac3Audio")
__all__ = list(_ESINDEX + _REMUX + _FRAGMENT + _CODECCONFIG + _HEVCCONFIG + _SAMPLEAES + _CAPTIONS + _MP4DEMUX + _CBCS
               + _CENC + _PACKEDAUDIO + _MPEGAUDIO + _AC3AUDIO)


def __getattr__(name):
    if name in _ESINDEX:
        from . import esindex

        return getattr(esindex, name)
    if name in _REMUX:
        from . import remux

        return getattr(remux, name)
    if name in _FRAGMENT:
        from . import fragment

        return getattr(fragment, name)
    if name in _CODECCONFIG:
        from . import codecconfig

        return getattr(codecconfig, name)
    if name in _HEVCCONFIG:
        from . import hevcconfig

        return getattr(hevcconfig, name)
    if name in _SAMPLEAES:
        from . import sampleaes

        return getattr(sampleaes, name)
    if name in _CAPTIONS:
        from . import captions

        return getattr(captions, name)
    if name in _MP4DEMUX:
        from . import mp4demux

        return getattr(mp4demux, name)
    if name in _CBCS:
        from . import cbcs

        return getattr(cbcs, name)
    if name in _CENC:
        from . import cenc

        return getattr(cenc, name)
    if name in _PACKEDAUDIO:
        from . import packedaudio

        return getattr(packedaudio, name)
    if name in _MPEGAUDIO:
        from . import mpegaudio

        return getattr(mpegaudio, name)
    if name in _AC3AUDIO:
        from . import ac3audio

        return getattr(ac3audio, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
