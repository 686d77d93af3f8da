"""Batched segment ops (``aes``, ``crc``, ``segment``, ``tsdemux``, ``esindex``, ``remux``,
``codecconfig``): import the submodule you need.  The entry points of the sample index, of the
remux and of the codec configuration are also reachable from the package (``ops.index_batch``,
``ops.EsIndex``, ``ops.remux_batch``, ``ops.Remuxed``, ``ops.config_batch``, ``ops.CodecConfig``),
resolved on first use."""

_ESINDEX = ("index_batch", "EsIndex")
_REMUX = ("remux_batch", "Remuxed")
_CODECCONFIG = ("config_batch", "CodecConfig")
__all__ = list(_ESINDEX + _REMUX + _CODECCONFIG)


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
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
