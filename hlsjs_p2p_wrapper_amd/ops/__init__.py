"""Batched segment ops (``aes``, ``crc``, ``segment``, ``tsdemux``, ``esindex``): import the
submodule you need.  The sample index's entry points are also reachable from the package
(``ops.index_batch``, ``ops.EsIndex``), resolved on first use."""

_ESINDEX = ("index_batch", "EsIndex")
__all__ = list(_ESINDEX)


def __getattr__(name):
    if name in _ESINDEX:
        from . import esindex

        return getattr(esindex, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
