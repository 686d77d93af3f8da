"""Batched segment ops (``aes``, ``crc``, ``segment``, ``tsdemux``, ``esindex``, ``remux``,
``codecconfig``, ``hevcconfig``, ``sampleaes``, ``captions``): import the submodule you need.  The
entry points of the sample index, of the remux, of the two codec configurations, of the SAMPLE-AES
decrypt and of the caption extraction are also reachable from the package (``ops.index_batch``,
``ops.EsIndex``, ``ops.remux_batch``,
``ops.Remuxed``, ``ops.config_batch``, ``ops.CodecConfig``, ``ops.hevc_config_batch``,
``ops.HevcConfig``, ``ops.sample_decrypt_batch``, ``ops.SampleAes``, ``ops.caption_batch``,
``ops.Captions``), resolved on first use."""

_ESINDEX = ("index_batch", "EsIndex")
_REMUX = ("remux_batch", "Remuxed")
_CODECCONFIG = ("config_batch", "CodecConfig")
_HEVCCONFIG = ("hevc_config_batch", "HevcConfig")
_SAMPLEAES = ("sample_decrypt_batch", "SampleAes")
_CAPTIONS = ("caption_batch", "Captions")
__all__ = list(_ESINDEX + _REMUX + _CODECCONFIG + _HEVCCONFIG + _SAMPLEAES + _CAPTIONS)


def __getattr__(name):
    if name in _ESINDEX:
        from . import esindex

        return getattr(esindex, name)
    if name in _REMUX:
        from . import remux

        return getattr(remux, name)
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
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
