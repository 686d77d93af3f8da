"""Batched segment ops (``aes``, ``crc``, ``segment``, ``tsdemux``, ``esindex``, ``remux``): import the
submodule you need.  The entry points of the sample index and of the remux are also reachable
from the package (``ops.index_batch``, ``ops.EsIndex``, ``ops.remux_batch``, ``ops.Remuxed``),
resolved on first use."""

_ESINDEX = ("index_batch", "EsIndex")
_REMUX = ("remux_batch", "Remuxed")
__all__ = list(_ESINDEX + _REMUX)


def __getattr__(name):
    if name in _ESINDEX:
        from . import esindex

        return getattr(esindex, name)
    if name in _REMUX:
        from . import remux

        return getattr(remux, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
