"""Batched decrypt + demux stage between ``FRAG_LOADED`` and the buffer (hls.js's
decrypter + TS demuxer, moved onto the MI355X).

Every fragment loaded during one event-loop iteration — typically all fragments
completed by one swarm exchange round — is decrypted by ONE AES-CBC launch and demuxed
by ONE demux launch sequence, then a single small device->host copy of the per-segment
``info`` rows delivers timing/status to the players.  Payloads that are views of the
node's HBM arena are consumed in place (no copy); host payloads (default CDN loader) are
staged with one H2D copy.

A batch has one internal form, columns (:class:`_Columns`: source buffer, offsets, sizes,
encrypted flags, IVs, keys, expected CRCs), and one launch core, ``_launch_core``: it rejects
encrypted fragments that are not whole AES blocks, gives every fragment that asked for a CRC
check exactly one, and calls the backend (one native ``transmux_launch`` on the GPU, the host
kernels on CPU).  ``launch()`` (jobs submitted one by one) and ``launch_columns()`` (a fleet
rank's arrays) are adapters over it, and ``_rows`` gathers a completed batch's result rows
for ``complete()``, ``complete_arrays()`` and ``complete_columns()`` alike.

Fragmented-MP4 and packed-audio jobs are set aside in front of the columns and take one path of
their own, ``_launch_aside`` / ``_complete_aside``, told apart by :class:`_Mp4` and
:class:`_Packed`.  What the containers share is written once: ``_accepted`` (the reject rule),
``_cbc_work`` (the AES-128 decrypt and the demux work list), ``_group_steps`` (what follows a
group's demux), ``_ts_result`` / ``_attach`` (the MPEG-TS shaped result and what hangs off it).

The batching point is per (thread, device): the peer threads of an in-process swarm each
get their own pipeline.
"""
from __future__ import annotations

import threading
import time
from dataclasses import dataclass, field
from types import MappingProxyType
from typing import Any, Callable, Dict, List, Optional, Tuple

import numpy as np
import torch

from ..net.event_loop import get_event_loop
from ..ops import aes as _aes
from ..ops import crc as _crc
from ..ops import tsdemux as _ts
from ..ops._native import device as _native_device
from ..utils.trace import PhaseTimer

ALIGN = 256
# the errors of a fragment's result (``ValueError``)
ERR_BLOCKS = "encrypted payload is not a multiple of 16 bytes"
ERR_PADDING = "decryption failed (bad PKCS#7 padding)"
ERR_CRC = "received segment failed its CRC check"


class TransmuxJob:
    """One fragment to transmux: ``payload`` (torch uint8 tensor on any device / numpy /
    bytes), the AES-128 ``key`` and ``iv`` (``None``: clear), ``callback(result)``.  A
    ``METHOD=SAMPLE-AES`` fragment is not CBC-encrypted as a whole: its ``key`` and ``iv`` stay
    ``None`` and ``sample_key`` / ``sample_iv`` (16 bytes each) are set instead.  A plain
    slotted class: one is built per fragment, and a dataclass ``__init__`` stays interpreted
    code inside the compiled module.  ``mp4`` (an ``Mp4Init``): the payload is a fragmented-MP4 media
    segment of that init segment's tracks, not MPEG-TS (``docs/FMP4DEMUX.md``): the batch demuxes it
    where it lies and ``remux`` is ignored (the fragment already is fMP4).  ``sample_key`` with ``mp4``
    asks for the ``cbcs`` decrypt (``docs/CBCS.md``) or the ``cenc`` decrypt (``docs/CENC.md``): it is
    accepted when the init segment has a track protected under one of the two schemes, which decides
    the decrypt that runs (``scheme``; the key of ``sample_iv`` serves a track without an IV of its
    own), and the result's ``data`` and views are then those of the decrypted copy.  ``packed_audio``:
    the payload is a packed-audio segment, ID3v2 tags in front of raw ADTS frames
    (``docs/PACKEDAUDIO.md``): the batch demuxes it where it lies and the result has the shape of an
    MPEG-TS fragment's, with ``container`` ``"aac"`` and ``packed_audio``; not with ``mp4`` or
    ``sample_key``."""

    __slots__ = ("payload", "key", "iv", "callback", "frag", "verify", "index", "remux", "sample_key", "sample_iv",
                 "captions", "mp4", "scheme", "fragment", "sequence_number", "time_base", "time_ref", "anchor",
                 "packed_audio", "aside")

    def __init__(self, payload: Any, key: Optional[bytes], iv: Optional[bytes],
                 callback: Callable[[Dict[str, Any]], None], frag: Any = None, verify: Any = None,
                 index: bool = False, remux: bool = False, sample_key: Optional[bytes] = None,
                 sample_iv: Optional[bytes] = None, captions: bool = False, mp4: Any = None,
                 fragment: bool = False, sequence_number: int = 0, time_base: int = 0, time_ref: int = -1,
                 anchor: bool = False, packed_audio: bool = False) -> None:
        # ``fragment`` (implies ``remux``): the batch also writes both moof boxes of this fragment in
        # front of its mdat boxes (ops/fragment.py, docs/FRAGMENT.md) and the tracks of its ``fmp4``
        # gain ``fragment``, ``moof_view`` and ``tfdt``.  ``sequence_number`` goes into the mfhd;
        # the tfdt values are relative to ``time_base`` and unwrapped against ``time_ref`` (90 kHz,
        # -1: none), or with ``anchor`` the fragment's first stamp lands on ``time_ref`` and the base
        # that follows comes back as ``fmp4["time_base"]``
        if fragment and anchor and time_ref < 0:
            raise ValueError("TransmuxJob: an anchored fragment needs a time_ref >= 0")
        if packed_audio and mp4 is not None:
            raise ValueError("TransmuxJob: a fragment is packed audio or fragmented MP4, not both")
        if packed_audio and sample_key is not None:
            raise ValueError("TransmuxJob: SAMPLE-AES packed audio is not supported")
        self.packed_audio = packed_audio
        # mp4 or packed_audio: the pipeline sets the job aside in front of the MPEG-TS columns
        self.aside = packed_audio or mp4 is not None
        remux = remux or fragment
        self.fragment = fragment
        self.sequence_number, self.time_base, self.time_ref, self.anchor = sequence_number, time_base, time_ref, anchor
        self.payload = payload
        self.key = key
        self.iv = iv
        self.callback = callback
        self.frag = frag
        self.verify = verify
        # a received segment's pending CRC check (agent/node.py VerifyTicket: ``expect``,
        # ``report(ok)``): the batch verifies the bytes -- fused into the decrypt -- reports the
        # outcome, and a fragment that fails gets a ``verify_failed`` error result
        if (sample_key is None) != (sample_iv is None):
            raise ValueError("TransmuxJob: sample_key and sample_iv go together")
        self.sample_key = sample_key
        self.sample_iv = sample_iv
        # set: the batch decrypts this fragment's protected NAL units and ADTS frames in its ES
        # behind the sample index (ops/sampleaes.py) and its result gains ``sample_aes``
        self.index = index or remux or sample_key is not None or captions
        # True: the batch also indexes this fragment's NAL units, access units and ADTS frames
        # (ops/esindex.py) and its result gains ``samples``
        self.remux = remux
        # True (implies ``index``): the batch also remuxes this fragment to fMP4 samples and mdat
        # boxes (ops/remux.py) and its result gains ``fmp4``
        self.captions = captions
        # True (implies ``index``): the batch also extracts the CEA-608/708 caption data of this
        # fragment's SEI NAL units (ops/captions.py) and its result gains ``captions``
        self.scheme = None  # "cbcs" / "cenc": the decrypt of a fragmented-MP4 job that asked
        if mp4 is not None and sample_key is not None:
            schemes = [getattr(getattr(t, "protection", None), "scheme", None) for t in getattr(mp4, "tracks", ())]
            if "cbcs" in schemes and "cenc" in schemes:
                raise ValueError("TransmuxJob: an init segment with a cbcs and a cenc track is not supported")
            if "cbcs" not in schemes and "cenc" not in schemes:
                raise ValueError("TransmuxJob: SAMPLE-AES (cbcs) fragmented MP4 is not supported")
            self.scheme = "cbcs" if "cbcs" in schemes else "cenc"
            if key is not None:
                raise ValueError("TransmuxJob: a fragmented-MP4 fragment is AES-128 or SAMPLE-AES, not both")
        self.mp4 = mp4
        if mp4 is not None:  # the fragment already is fMP4: no remux, and none that implies the index
            self.remux = self.fragment = False
            self.index = bool(index or captions)

    def __repr__(self) -> str:
        return f"TransmuxJob(key={'set' if self.key else None}, frag={self.frag!r})"


def _as_tensor(payload: Any) -> torch.Tensor:
    if isinstance(payload, torch.Tensor):
        return payload if payload.dim() == 1 else payload.reshape(-1)  # arena slices are 1-D already
    if isinstance(payload, np.ndarray):
        return torch.from_numpy(np.ascontiguousarray(payload.reshape(-1)).view(np.uint8))
    if isinstance(payload, (bytes, bytearray, memoryview)):
        return torch.frombuffer(bytearray(payload), dtype=torch.uint8)
    raise TypeError(f"unsupported payload type {type(payload)!r}")


def _align(n: int) -> int:
    return (n + ALIGN - 1) // ALIGN * ALIGN


def _layout(caps: np.ndarray) -> Tuple[np.ndarray, int]:
    """ALIGN-ed offsets of consecutive buffers of ``caps`` bytes, and their total size."""
    sizes = (caps + (ALIGN - 1)) // ALIGN * ALIGN
    ends = np.cumsum(sizes)
    return ends - sizes, int(ends[-1])


def _np(x) -> np.ndarray:
    return x.numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


def _to_host(t):
    """A small device tensor on its way into pinned host memory (async, on the current
    stream: readable after the batch's event); a CPU tensor as numpy, a numpy array as it is."""
    if not isinstance(t, torch.Tensor):
        return t
    if t.device.type == "cpu":
        return t.numpy()
    h = torch.empty(t.shape, dtype=t.dtype, pin_memory=True)
    h.copy_(t, non_blocking=True)
    return h


def _accepted(enc: np.ndarray, nb: np.ndarray) -> np.ndarray:
    """bool[n], the reject rule: an encrypted row must be a positive number of whole AES blocks."""
    return ~(enc & ((nb <= 0) | (nb % 16 != 0)))


def _enc_iv(jobs: List[TransmuxJob]) -> Tuple[List[int], np.ndarray, np.ndarray]:
    """The AES-128 jobs among ``jobs``: their positions, ``enc`` bool[n] and ``iv`` uint8[n, 16]."""
    n = len(jobs)
    e = [i for i, j in enumerate(jobs) if j.key is not None]
    enc = np.zeros(n, dtype=bool)
    iv = np.zeros((n, 16), dtype=np.uint8)
    if e:
        enc[e] = True
        iv[e] = np.frombuffer(b"".join(bytes(jobs[i].iv) for i in e), dtype=np.uint8).reshape(-1, 16)
    return e, enc, iv


def _frag_params(jobs: List[TransmuxJob]) -> Tuple[Optional[np.ndarray], Optional[np.ndarray]]:
    """``(fragment bool[n], frag_params int64[n, 4])`` of ``jobs`` (``_Columns``), ``(None, None)``
    when no job asked for its moof boxes."""
    asked = [i for i, j in enumerate(jobs) if j.fragment]
    if not asked:
        return None, None
    params = np.tile(np.array([0, 0, -1, 0], dtype=np.int64), (len(jobs), 1))
    params[asked] = [(jobs[i].sequence_number, jobs[i].time_base, jobs[i].time_ref, int(bool(jobs[i].anchor)))
                     for i in asked]
    return _mask(len(jobs), asked), params


def _by_scheme(work: List[Tuple[Any, ...]], jobs: List[TransmuxJob]) -> List[Tuple[Any, ...]]:
    """The work tuples of :meth:`MediaPipeline._cbc_work` with the rows of each grouped by the
    decrypt they asked for: none, ``cbcs``, ``cenc`` (an AES-128 row asks for none)."""
    out = []
    for rows, buf, offs, lens, caps in work:
        scheme = np.array([(None, "cbcs", "cenc").index(jobs[i].scheme) for i in rows.tolist()])
        for s in np.unique(scheme).tolist():
            m = scheme == s
            out.append((rows, buf, offs, lens, caps) if m.all() else (rows[m], buf, offs[m], lens[m], caps[m]))
    return out


def _failed(error: BaseException, container: Optional[str] = None) -> Dict[str, Any]:
    """The result of a fragment that got no row; ``container``: of a job that was set aside."""
    return {"error": error, "status": -1, **({} if container is None else {"container": container})}


class _Columns:
    """A batch in its one internal form.  Fragment ``i`` is ``src[offs[i] : offs[i] + nb[i]]``
    (16-byte aligned offsets); ``enc[i]``: AES-128-CBC with ``iv[i]`` and, for the device,
    round keys ``drk[i]`` (``ops.aes.round_keys_le``) or, for the host, the raw key
    ``keys[i]``; ``expect`` (``None``: no checks) holds the CRC-32 fragment i's bytes must
    have, ``-1`` for no check; ``index`` (``None``: nobody) marks the fragments whose samples
    are to be indexed, ``remux`` those to be remuxed as well, ``sample`` (a subset of ``index``)
    those whose ES is SAMPLE-AES protected, with ``sample_keys[i]`` / ``sample_ivs[i]``, ``captions``
    (a subset of ``index``) those whose caption data is to be extracted, ``fragment`` (a subset of
    ``remux``) those whose moof boxes are to be written, with ``frag_params[i]`` = (sequence number,
    time base, time reference, anchor)."""

    __slots__ = ("src", "offs", "nb", "enc", "iv", "drk", "keys", "expect", "index", "remux", "sample", "sample_keys",
                 "sample_ivs", "captions", "fragment", "frag_params")

    def __init__(self, src: torch.Tensor, offs: np.ndarray, nb: np.ndarray, enc: np.ndarray, iv: np.ndarray,
                 drk: Optional[np.ndarray] = None, keys: Any = None, expect: Optional[np.ndarray] = None,
                 index: Optional[np.ndarray] = None, remux: Optional[np.ndarray] = None,
                 sample: Optional[np.ndarray] = None, sample_keys: Any = None, sample_ivs: Any = None,
                 captions: Optional[np.ndarray] = None, fragment: Optional[np.ndarray] = None,
                 frag_params: Optional[np.ndarray] = None) -> None:
        self.src = src      # uint8 tensor on the pipeline's device
        self.offs = offs    # int64[n]
        self.nb = nb        # int64[n]
        self.enc = enc      # bool[n]
        self.iv = iv        # uint8[n, 16]
        self.drk = drk      # uint32[n, 44]
        self.keys = keys    # n raw 16-byte keys (a list or uint8[n, 16]); read only where enc is set
        self.expect = expect  # int64[n]
        self.index = index  # bool[n]
        self.remux = remux  # bool[n], a subset of index
        self.sample = sample  # bool[n], a subset of index
        self.sample_keys = sample_keys  # n raw 16-byte keys (None where sample is not set)
        self.sample_ivs = sample_ivs
        self.captions = captions  # bool[n], a subset of index
        self.fragment = fragment  # bool[n], a subset of remux
        self.frag_params = frag_params  # int64[n, 4]; rows that did not ask hold (0, 0, -1, 0)


class MediaPipeline:
    def __init__(self, device: torch.device, loop=None) -> None:
        self.device = torch.device(device)
        if self.device.type == "cuda" and self.device.index is None:
            # "cuda" != "cuda:0": an index-less device would fail the in-place staging check
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.loop = loop or get_event_loop()
        self._jobs: List[TransmuxJob] = []
        self._any_aside = False  # a submitted job is fragmented MP4 or packed audio: launch() sets those aside
        self._scheduled = False
        self.segments = 0
        self.bytes_in = 0
        self.batches = 0
        self.timer = PhaseTimer()
        self._free_events: List[Any] = []  # timing events (start / end of each batch on the device)
        # event-loop players flush at the end of the loop iteration; a throughput driver
        # sets auto_flush=False and overlaps launch() / complete() of consecutive batches
        self.auto_flush = True

    def submit(self, job: TransmuxJob) -> None:
        self._jobs.append(job)
        if job.aside:
            self._any_aside = True
        if self.auto_flush and not self._scheduled:
            self._scheduled = True
            self.loop.call_soon(self.flush)

    def flush(self) -> None:
        """Synchronous batch: launch the kernels for everything submitted, then complete."""
        self._scheduled = False
        self.complete(self.launch())

    def launch(self) -> Optional["_Batch"]:
        """Enqueue decrypt + demux for every submitted job; the host does not wait."""
        jobs, self._jobs = self._jobs, []
        if not jobs:
            return None
        aside: Any = ()
        if self._any_aside:  # fragmented-MP4 and packed-audio jobs take their own path, in front of the columns
            self._any_aside = False
            parts = [(_Mp4, [j for j in jobs if j.mp4 is not None]), (_Packed, [j for j in jobs if j.packed_audio])]
            aside = [self._launch_aside(kind, kj) for kind, kj in parts if kj]
            jobs = [j for j in jobs if not j.aside]
            if not jobs:
                return _Batch([], groups=[], n=0, aside=aside)
        try:
            b = self._launch_core(self._job_columns(jobs))
        except Exception as e:  # deliver the failure to every job of the batch
            return _Batch(jobs, groups=[], error=e, n=len(jobs), aside=aside)
        b.jobs = jobs
        b.aside = aside
        return b

    def complete(self, batch: Optional["_Batch"]) -> None:
        """Wait for a launched batch and run the per-fragment callbacks."""
        if batch is None:
            return
        if batch.aside:
            for part in batch.aside:
                self._complete_aside(part)
            if not batch.jobs:
                return
        if batch.error is not None:
            for j in batch.jobs:  # (a pending receive check is left to the node's own sweep)
                j.callback({"error": batch.error})
            return
        results = self._complete(batch)
        if batch.expect_mask is not None:  # deferred receive checks: report, drop failed results
            ok = self._verified(batch, len(batch.jobs))
            for i in np.flatnonzero(batch.expect_mask).tolist():
                batch.jobs[i].verify.report(bool(ok[i]))
                if not ok[i]:
                    results[i] = dict(_failed(ValueError(ERR_CRC)), verify_failed=True)
        t = time.perf_counter()
        for j, r in zip(batch.jobs, results):
            j.callback(r)
        self.timer.add("callbacks", time.perf_counter() - t)

    # ------------------------------------------------------------------ device events
    def _event(self):
        """A recorded timing event on the current stream (recycled: a fresh event costs
        ~5 us of host time)."""
        ev = self._free_events.pop() if self._free_events else torch.cuda.Event(enable_timing=True)
        ev.record()
        return ev

    def _wait(self, b: "_Batch") -> None:
        """Host wait for a batch's device work; its device time goes to ``dev_transmux``."""
        if b.event is None:
            return
        b.event.synchronize()
        if b.start is not None:
            self.timer.add("dev_transmux", b.start.elapsed_time(b.event) / 1e3)
            self._free_events.append(b.start)
            b.start = None
        self._free_events.append(b.event)
        b.event = None

    # ------------------------------------------------------------------ batch
    def _stage(self, tensors: List[torch.Tensor], sizes: List[int]) -> Tuple[torch.Tensor, List[int]]:
        """One source buffer + offsets: in place when every payload is a view of the same
        device storage (the HBM arena), otherwise one staging copy.  Same-storage check: one
        ``data_ptr()`` per payload, every view inside the first payload's allocation
        (allocations never overlap), instead of a storage object per payload."""
        dev = self.device
        t0 = tensors[0]
        if t0.device == dev:
            cuda = dev.type == "cuda"
            storage = t0.untyped_storage()
            base_ptr, cap = storage.data_ptr(), storage.nbytes()
            offs = [t.data_ptr() - base_ptr for t in tensors]
            if all(o >= 0 and o + n <= cap and o % 16 == 0 and t.is_cuda == cuda
                   for o, n, t in zip(offs, sizes, tensors)):
                base = torch.empty(0, dtype=torch.uint8, device=dev).set_(storage, 0, (cap,))
                return base, offs
        offs, pos = [], 0
        for t in tensors:
            offs.append(pos)
            pos += _align(t.numel())
        buf = torch.empty(pos + ALIGN, dtype=torch.uint8, device=dev)
        for o, t in zip(offs, tensors):
            buf[o:o + t.numel()].copy_(t, non_blocking=True)
        return buf, offs

    def _stage_jobs(self, jobs: List[TransmuxJob]) -> Tuple[torch.Tensor, np.ndarray, np.ndarray]:
        """The payloads of ``jobs`` in one source buffer (:meth:`_stage`): ``(src, offs, nb)``."""
        tensors = [_as_tensor(j.payload) for j in jobs]
        sizes = [t.numel() for t in tensors]
        src, src_offs = self._stage(tensors, sizes)
        return src, np.asarray(src_offs, dtype=np.int64), np.asarray(sizes, dtype=np.int64)

    def _job_columns(self, jobs: List[TransmuxJob]) -> _Columns:
        """The submitted jobs as columns: payloads staged into one source buffer; one key per
        stream (the usual case) is expanded once."""
        t0 = time.perf_counter()
        cuda = self.device.type == "cuda"
        src, offs, nb = self._stage_jobs(jobs)
        n = len(jobs)
        e, enc, iv = _enc_iv(jobs)
        drk = np.zeros((n, 44), dtype=np.uint32) if cuda else None
        if e and cuda:  # (the host decrypt expands the raw keys itself)
            k0 = jobs[e[0]].key
            if all(jobs[i].key is k0 or jobs[i].key == k0 for i in e):
                drk[e] = _aes.round_keys_le(bytes(k0))
            else:
                drk[e] = [_aes.round_keys_le(bytes(jobs[i].key)) for i in e]
        expect = None
        v = [i for i, j in enumerate(jobs) if j.verify is not None]
        if v:
            expect = np.full(n, -1, dtype=np.int64)
            expect[v] = [jobs[i].verify.expect & 0xFFFFFFFF for i in v]
        cols = _Columns(src, offs, nb, enc, iv, drk=drk,
                        keys=None if cuda else [j.key for j in jobs], expect=expect,
                        index=_mask(n, [i for i, j in enumerate(jobs) if j.index]),
                        remux=_mask(n, [i for i, j in enumerate(jobs) if j.remux]),
                        sample=_mask(n, [i for i, j in enumerate(jobs) if j.sample_key is not None]),
                        sample_keys=[j.sample_key for j in jobs], sample_ivs=[j.sample_iv for j in jobs],
                        captions=_mask(n, [i for i, j in enumerate(jobs) if j.captions]))
        cols.fragment, cols.frag_params = _frag_params(jobs)
        self.timer.add("stage", time.perf_counter() - t0)
        return cols

    def launch_columns(self, src: torch.Tensor, offs: np.ndarray, nbytes: np.ndarray, enc: np.ndarray,
                       drk: np.ndarray, iv: np.ndarray, tag: Any = None, keys: Optional[np.ndarray] = None,
                       expect: Optional[np.ndarray] = None) -> Optional["_Batch"]:
        """A batch given as columns (a fleet rank: no job object per fragment), handed to the
        launch core as it is.  Fragment ``i`` is ``src[offs[i] : offs[i] + nbytes[i]]`` (the
        node's HBM arena, 16-byte aligned offsets); ``enc[i]``: AES-128-CBC with round keys
        ``drk[i]`` (44 little-endian words, ``ops.aes.round_keys_le``) and ``iv[i]``; on CPU the
        host decrypt reads the raw 16-byte ``keys[i]`` instead, and without ``keys`` every
        fragment is taken as clear.  ``expect[i] >= 0``: fragment i's bytes must have that
        CRC-32 (a peer's trailer, verified here instead of by the node); :meth:`complete_columns`
        reports the outcome.  ``tag`` comes back from :meth:`complete_columns`.  No fragment is
        indexed, sample-decrypted, remuxed or searched for captions (``TransmuxJob.index`` /
        ``.sample_key`` / ``.remux`` / ``.captions`` are the job form's)."""
        n = len(offs)
        if n == 0:
            return None
        cuda = self.device.type == "cuda"
        enc = np.asarray(enc, dtype=bool)
        if not cuda and keys is None:
            enc = np.zeros(n, dtype=bool)
        if expect is not None:
            expect = np.ascontiguousarray(expect, dtype=np.int64)
            if not (expect >= 0).any():
                expect = None
        col = np.ascontiguousarray
        return self._launch_core(
            _Columns(src, col(offs, dtype=np.int64), col(nbytes, dtype=np.int64), enc, col(iv, dtype=np.uint8),
                     drk=col(drk, dtype=np.uint32) if cuda else None, keys=keys, expect=expect), tag)

    # ------------------------------------------------------------------ the launch core
    def _launch_core(self, c: _Columns, tag: Any = None) -> "_Batch":
        """Enqueue one batch; every index of the returned batch is a row of ``c``.

        * An encrypted row that is not a positive number of whole AES blocks is rejected: it
          gets no decrypt or demux row.
        * Every row with ``expect >= 0`` gets exactly one CRC check: on the GPU an accepted
          encrypted row is checked by the decrypt that reads it (the CRC fused into
          ``aes_cbc.hip``), every other row -- clear, rejected, and all of them on CPU -- by
          ``ops.crc.crc32_batch``.  ``expect_mask`` records who asked, so :meth:`_verified`
          fails a row no check covered.
        * GPU: ONE native call (``kernels/transmux.cpp``): descriptor math, one staging H2D,
          AES-CBC decrypt, demux per group (encrypted, then clear, each in row order), D2H of
          the info rows.  CPU: the host kernels, the same groups."""
        t1 = time.perf_counter()
        cuda = self.device.type == "cuda"
        n = len(c.offs)
        self.segments += n
        self.bytes_in += int(c.nb.sum())
        self.batches += 1
        ok = _accepted(c.enc, c.nb)
        rows = np.flatnonzero(ok)
        verify: List[Any] = []
        mask = ex = None
        if c.expect is not None:
            mask = c.expect >= 0
            fuse = mask & c.enc & ok if cuda else np.zeros(n, dtype=bool)
            side = np.flatnonzero(mask & ~fuse)
            if len(side):
                _, okd = _crc.crc32_batch(c.src, c.offs[side], c.nb[side],
                                          expect=(c.expect[side] & 0xFFFFFFFF).tolist())
                verify.append((side, _to_host(okd)))
            if fuse.any():
                ex = np.where(fuse, c.expect, -1)[rows]
        groups: List[_Group] = []
        keep = ev0 = None
        if not len(rows):  # nothing to decrypt or demux (the CRC checks above still run)
            pass
        elif cuda:
            take = (lambda a: a) if len(rows) == n else (lambda a: a[rows])
            td0, isb = _aes.device_tables(self.device)
            cw, ctab = _crc.fused_consts(self.device) if ex is not None else (None, None)
            ev0 = self._event()
            out, dec, host_block, fused = _native_device().transmux_launch(
                c.src, take(c.offs), take(c.nb), take(c.enc).astype(np.uint8), take(c.drk), take(c.iv), td0, isb,
                _ts.DEFAULT_MAX_PES, ex, cw, ctab)
            keep = (dec, host_block)
            for gidx, info, pes, es, es_offs, hinfo, hlens in out:
                groups.append(_Group(rows[gidx], _ts.DemuxResult(info, pes, es, es_offs), hinfo, hlens))
            if fused is not None:  # rows of the launch -> rows of the batch
                verify.append((rows[fused[0]], fused[1]))
        else:
            groups = self._host_groups(c, rows)
        for g in groups:
            self._group_steps(g, c)
        # completing the batch is the stage's only sync: one event after everything enqueued
        ev = self._event() if cuda and (groups or verify) else None
        self.timer.add("launch", time.perf_counter() - t1)
        return _Batch(None, groups=groups, event=ev, keep=keep, tag=tag, n=n, start=ev0, verify=verify or None,
                      expect_mask=mask)

    def _group_steps(self, g: "_Group", c: _Columns) -> None:
        """The steps behind a group's demux, each one call on the same stream when a row of the group
        asked for it in ``c``, its small tables on their way to the host before the batch's event."""
        rows = g.rows
        if g.ix is None:
            # the sample index (a container whose demux brings its own has it already): one
            # ``index_batch`` call; ``sample``, ``captions`` and ``remux`` are subsets of ``index``
            if not _any(c.index, rows):
                return
            from ..ops import esindex as _esx

            g.ix = _esx.index_batch(g.res, c.nb[rows])
            g.sinfo = _to_host(g.ix.sinfo)
        ix, caps = g.ix, c.nb[rows]
        # ... the SAMPLE-AES decrypt, in front of the captions, the remux and the two configuration
        # calls, which then read the decrypted ES; rows that did not ask are not enabled
        if _any(c.sample, rows):
            from ..ops import sampleaes as _sa

            il = rows.tolist()
            g.sa = sa = _sa.sample_decrypt_batch(g.res, ix, caps, [c.sample_keys[i] for i in il],
                                                 [c.sample_ivs[i] for i in il], c.sample[rows].tolist())
            g.sainfo = _to_host(sa.sainfo)
        # ... the caption data (rows that did not ask are not enabled)
        if _any(c.captions, rows):
            from ..ops import captions as _cc

            g.cc = cc = _cc.caption_batch(g.res, ix, caps, enable=c.captions[rows].tolist())
            g.ccinfo = _to_host(cc.ccinfo)
        if _any(c.remux, rows):  # ... and the remux, with the moof boxes where a row asked for them
            self._launch_remux(g, caps, c.frag_params[rows] if _any(c.fragment, rows) else None)

    def _launch_remux(self, g: "_Group", caps: np.ndarray, frag_params: Optional[np.ndarray]) -> None:
        """The remux of an indexed group in which a row asked for it: one ``remux_batch`` call behind
        the index, its three tables on their way to the host; ``frag_params`` (the group's rows of
        (sequence number, time base, time reference, anchor), ``None``: no row asked for its moof
        boxes) adds one ``fragment_batch`` call behind it; then the two configuration calls.  Directly
        behind the remux stands one ``mpeg_audio_batch`` call (docs/MPEGAUDIO.md): the audio codec is
        only known on the device, so the launch is unconditional, and a segment whose audio is not
        MPEG audio exits at once and keeps every byte of the remux.  Behind it stands one
        ``ac3_audio_batch`` call (docs/AC3AUDIO.md) of the same shape for AC-3 / E-AC-3; its ``mpainfo``
        holds the rows of both ops and is what ``fragment_batch`` takes."""
        from ..ops import ac3audio as _ac3
        from ..ops import mpegaudio as _mpa
        from ..ops import remux as _rmx

        ix = g.ix
        # a group in which any row asked for its moof boxes leaves room for them in every
        # region (so a row that did not ask sees a larger ``audio_box_offset``, nothing else)
        # and gets one ``fragment_batch`` call behind the remux, its ``finfo`` rows on the
        # same way to the host (docs/FRAGMENT.md)
        fragment = frag_params is not None
        headroom = gap = 0
        if fragment:
            from ..ops import fragment as _frg

            headroom = _frg.frag_headroom(g.res.pes.shape[2])
            gap = _frg.frag_audio_gap(_rmx.DEFAULT_MAX_AFRAMES)
        out_offs, size = _rmx.layout_out(caps, ix.nal.shape[1], headroom=headroom, audio_gap=gap)
        g.rx = rx = _rmx.remux_batch(g.res, ix, caps,
                                     torch.empty(size + ALIGN, dtype=torch.uint8, device=g.res.es.device),
                                     out_offs, audio_gap=gap, headroom=headroom)
        # in front of the copies to the host: the op rewrites rinfo and asamples of its segments
        g.ma = ma = _mpa.mpeg_audio_batch(g.res, rx, caps)
        g.da = da = _ac3.ac3_audio_batch(g.res, rx, caps, mpeg_audio=ma)
        g.rinfo, g.vsamples, g.asamples = _to_host(rx.rinfo), _to_host(rx.vsamples), _to_host(rx.asamples)
        g.mpainfo = _to_host(ma.mpainfo)
        g.ac3info = _to_host(da.ac3info)
        if fragment:
            fp = frag_params
            g.fr = fr = _frg.fragment_batch(rx, ix, fp[:, 0], time_base=fp[:, 1], time_ref=fp[:, 2],
                                            anchor=fp[:, 3] != 0, mpeg_audio=da)
            g.finfo = _to_host(fr.finfo)
        # ... and what the init segments are built from: one ``config_batch`` call behind the
        # remux, its two tensors on the same way to the host (docs/INITSEGMENT.md)
        from ..ops import codecconfig as _cfg

        g.cfg = cfg = _cfg.config_batch(g.res, ix, caps)
        g.cinfo, g.ps = _to_host(cfg.cinfo), _to_host(cfg.ps)
        # ... and one ``hevc_config_batch`` call behind it for the HEVC segments among them:
        # the codec is only known on the device, so the launch is unconditional and the
        # workgroup of any other segment exits at once
        from ..ops import hevcconfig as _hcfg

        g.hcfg = hcfg = _hcfg.hevc_config_batch(g.res, ix, caps)
        g.hvinfo, g.hps = _to_host(hcfg.hinfo), _to_host(hcfg.hps)

    def _cbc_work(self, c: _Columns, rows: np.ndarray) -> List[Tuple[Any, ...]]:
        """The demux work list of the accepted ``rows`` of ``c``, ``(rows, buf, offs, lens, caps)``
        each: the encrypted rows behind ONE ``ops.aes.cbc_decrypt_batch`` call (raw keys ``c.keys``)
        into a freshly laid-out buffer, then the clear rows where they lie."""
        work = []
        e, cl = rows[c.enc[rows]], rows[~c.enc[rows]]
        if len(e):
            caps = c.nb[e]
            dec_offs, size = _layout(caps)
            dec = torch.empty(size + ALIGN, dtype=torch.uint8, device=self.device)
            out_len = _aes.cbc_decrypt_batch(c.src, c.offs[e], caps, [bytes(c.keys[i]) for i in e.tolist()], c.iv[e],
                                             dec, dec_offs)
            work.append((e, dec, dec_offs, out_len, caps))
        if len(cl):
            work.append((cl, c.src, c.offs[cl], c.nb[cl], c.nb[cl]))
        return work

    def _host_groups(self, c: _Columns, rows: np.ndarray) -> List["_Group"]:
        """The host backend: :meth:`_cbc_work`, then ``ops.tsdemux.demux_batch`` per group, like the
        native call's groups."""
        groups = []
        for idx, buf, offs, lens, caps in self._cbc_work(c, rows):
            es_offs, size = _layout(caps)
            es = torch.empty(size + ALIGN, dtype=torch.uint8, device=self.device)
            res = _ts.demux_batch(buf, offs, lens, es, es_offs, caps=caps)
            groups.append(_Group(idx, res, hlens=_to_host(lens), hinfo=_to_host(res.info)))
        return groups

    # ------------------------------------------------------------------ the jobs set aside
    def _launch_aside(self, kind: Any, jobs: List[TransmuxJob]) -> "_Aside":
        """Enqueue the jobs of one container that is not MPEG-TS (``kind``: :class:`_Mp4` or
        :class:`_Packed`): staging, :meth:`_cbc_work`, ``kind.demux`` per work tuple, then the steps
        of :meth:`_group_steps` that the container takes; every small table is on its way to pinned
        host memory in front of the event.  A failure is delivered to these jobs alone.  (A receive
        ticket, ``verify``, is not looked at here: the node's own sweep checks it later.)"""
        try:
            src, offs, nb = self._stage_jobs(jobs)
            n = len(jobs)
            self.segments += n
            self.bytes_in += int(nb.sum())
            _, enc, iv = _enc_iv(jobs)
            c = _Columns(src, offs, nb, enc, iv, keys=[j.key for j in jobs])
            if kind.captions:
                c.captions = _mask(n, [i for i, j in enumerate(jobs) if j.captions])
            if kind.remux:
                c.remux = _mask(n, [i for i, j in enumerate(jobs) if j.remux])
                c.fragment, c.frag_params = _frag_params(jobs)
            ok = _accepted(enc, nb)
            groups = []
            for work in _by_scheme(self._cbc_work(c, np.flatnonzero(ok)), jobs):
                g = kind.demux(jobs, *work)
                self._group_steps(g, c)
                groups.append(g)
            ev = self._event() if self.device.type == "cuda" and groups else None
            return _Aside(kind, jobs, groups, ev, None, np.flatnonzero(~ok))
        except Exception as e:  # deliver the failure to every job of this container in the batch
            return _Aside(kind, jobs, [], None, e, np.zeros(0, dtype=np.int64))

    def _complete_aside(self, b: "_Aside") -> None:
        """Wait for the jobs of a batch that were set aside as one container and run their callbacks."""
        name = b.kind.name
        if b.error is not None:
            for j in b.jobs:
                j.callback(_failed(b.error, name))
            return
        self._wait(b)
        results: List[Any] = [None] * len(b.jobs)
        for i in b.rejected.tolist():
            results[i] = _failed(ValueError(ERR_BLOCKS), name)
        for g in b.groups:
            for i, r in zip(g.rows.tolist(), b.kind.rows(g, b.jobs)):
                r["container"] = name
                results[i] = r
        for j, r in zip(b.jobs, results):
            j.callback(r)

    # ------------------------------------------------------------------ completion
    def _rows(self, batch: "_Batch") -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """Wait for a batch and gather its result rows: ``(rows int64[n, INFO_WORDS], plain
        int64[n], has_row bool[n])`` aligned with the batch's fragments: the demux info rows,
        the plaintext lengths, and whether the fragment has a row (False: rejected before
        launch; its ``plain`` is -1)."""
        n = batch.n
        rows = np.zeros((n, _ts.INFO_WORDS), dtype=np.int64)
        plain = np.full(n, -1, dtype=np.int64)
        has = np.zeros(n, dtype=bool)
        t3 = time.perf_counter()
        self._wait(batch)
        self.timer.add("wait_device", time.perf_counter() - t3)
        for g in batch.groups:
            k = len(g.rows)
            rows[g.rows] = _np(g.hinfo)[:k]
            plain[g.rows] = _np(g.hlens)[:k]
            has[g.rows] = True
        return rows, plain, has

    def complete_arrays(self, batch: Optional["_Batch"]):
        """Wait for a launched batch; return ``(jobs, rows, plain, has_row)``: :meth:`_rows`
        aligned with ``jobs``.  The columnar form a fleet node ships to its players without a
        Python object per word."""
        if batch is None:
            return [], None, None, None
        return (batch.jobs,) + self._rows(batch)

    def complete_columns(self, batch: "_Batch"):
        """Wait for a :meth:`launch_columns` batch: ``(tag, rows int64[n, INFO_WORDS], plain
        int64[n], has_row bool[n], verified bool[n])`` aligned with the launch columns
        (``verified[i]`` False: fragment i failed its ``expect`` CRC)."""
        rows, plain, has = self._rows(batch)
        return batch.tag, rows, plain, has, self._verified(batch, batch.n)

    @staticmethod
    def _verified(batch: "_Batch", n: int) -> np.ndarray:
        """Per fragment: passed its CRC check (True where none was asked); call after the wait.
        A fragment that asked for a check is True only if a check actually ran and passed."""
        out = np.ones(n, dtype=bool)
        if batch.expect_mask is not None:
            out[batch.expect_mask] = False
        for idx, ok in batch.verify or ():
            out[idx] = _np(ok).astype(bool)
        return out

    def _complete(self, b: "_Batch") -> List[Dict[str, Any]]:
        """The per-fragment results of a job batch, built from :meth:`_rows`."""
        rows, plain, has = self._rows(b)
        t4 = time.perf_counter()
        rl, pl = rows.tolist(), plain.tolist()
        results: List[Any] = [None] * b.n
        for i in np.flatnonzero(~has).tolist():  # rejected before launch
            results[i] = _failed(ValueError(ERR_BLOCKS))
        for g in b.groups:
            res = g.res
            es = res.es
            il = g.rows.tolist()
            for k, (i, base) in enumerate(zip(il, res.es_offs.tolist())):
                results[i] = _ts_result(res, es, k, rl[i], base, pl[i])
            if g.ix is not None:  # a job of this group asked for the sample index
                srows = _np(g.sinfo).tolist()
                for k, i in enumerate(il):
                    _attach(results[i], g, k, b.jobs[i], srows[k])
        self.timer.add("results", time.perf_counter() - t4)
        return results


def _ts_result(res, es, k, row, base, plain) -> "_Result":
    """The MPEG-TS shaped result of row ``k`` of the demux ``res`` (``es`` its ES buffer): ``row`` its
    info row, ``base`` its ES offset, ``plain`` its plaintext length (negative: the decrypt found bad
    padding).  The ES views (per class, at the row's offsets from ``base``) are built on first
    access: the buffer path only needs their byte counts, which the info row holds.  (Called per
    row of every batch: no annotations for the compiled module to check.)"""
    r = _Result(status=row[0], info=InfoRow(row), plain_bytes=plain, demux=res, index=k)
    r._es = (es, base, row[_VB], row[_AB], row[_IB], row[_AO], row[_IO])
    if plain < 0:
        r["error"] = ValueError(ERR_PADDING)
    return r


def _attach(r: Any, g: "_Group", k: int, job: TransmuxJob, srow: List[int]) -> None:
    """What hangs off the result of row ``k`` of the indexed group ``g``: the sample index, the remux,
    the SAMPLE-AES decrypt and the caption data, each where the group ran it and ``job`` asked."""
    if job.index:
        r["samples"] = Samples(srow, g.ix, k)
    if g.rx is not None and job.remux:
        r["fmp4"] = Fmp4(g, k, srow, g.fr is not None and job.fragment)
    if g.sa is not None and job.sample_key is not None:
        from ..ops.sampleaes import segment_view

        r["sample_aes"] = MappingProxyType(segment_view(_np(g.sainfo)[k]))
    if g.cc is not None and job.captions:
        r["captions"] = CaptionData(g, k)


class _Mp4:
    """What tells a container that is set aside apart (:meth:`MediaPipeline._launch_aside`): ``name``
    (the results' ``container``), the steps of ``_group_steps`` that its groups take (``captions``;
    ``remux`` with fragment and configuration), ``demux`` (a work tuple into a :class:`_Group` that
    brings its own index) and ``rows`` (the results of a finished group, in its order).

    Fragmented MP4 (docs/FMP4DEMUX.md): one ``mp4_demux_batch`` per group and, behind the demux of a
    ``cbcs`` or ``cenc`` group, one ``cbcs_decrypt_batch`` / ``cenc_decrypt_batch`` (docs/CBCS.md,
    docs/CENC.md), whose views then are those of the decrypted copy."""

    name, captions, remux = "mp4", True, False

    @staticmethod
    def demux(jobs, rows, buf, offs, lens, caps):
        from ..ops import mp4demux as _mp4

        il = rows.tolist()
        inits, scheme = [jobs[i].mp4 for i in il], jobs[il[0]].scheme
        md = _mp4.mp4_demux_batch(buf, offs, lens, inits, caps=caps)
        cb = None
        if scheme:  # out of place: buf may be the arena that peers are served from
            if scheme == "cbcs":
                from ..ops.cbcs import cbcs_decrypt_batch as decrypt
            else:
                from ..ops.cenc import cenc_decrypt_batch as decrypt
            cb = decrypt(md, inits, [jobs[i].sample_key for i in il], [jobs[i].sample_iv for i in il])
            md = cb.md
        g = _Group(rows, md.as_demux(), md=md, minfo=_to_host(md.minfo), hinfo=_to_host(md.info), ix=md.as_index(),
                   sinfo=_to_host(md.sinfo), emsg=_to_host(md.emsg), hlens=_to_host(lens))
        if cb is not None:
            g.cbinfo, g.scheme = _to_host(cb.cinfo), scheme
        return g

    @staticmethod
    def rows(g, jobs):
        from ..ops.cbcs import segment_view as cbcs_view
        from ..ops.cenc import segment_view as cenc_view
        from ..ops.mp4demux import EMSG, MINFO

        md = g.md
        minfo, info, sinfo, emsg, hlens = (_np(x) for x in (g.minfo, g.hinfo, g.sinfo, g.emsg, g.hlens))
        for k, i in enumerate(g.rows.tolist()):
            job, row, plain = jobs[i], minfo[k].tolist(), int(hlens[k])
            r = {"status": row[MINFO["status"]], "info": {n: row[s] for n, s in MINFO.items()},
                 "plain_bytes": plain, "init": job.mp4, "mp4": md, "index": k,
                 "video": Mp4TrackView(md, k, 0, row, info[k], job.mp4),
                 "audio": Mp4TrackView(md, k, 1, row, info[k], job.mp4),
                 "data": md.buf.narrow(0, int(md.offs[k]), max(plain, 0)),
                 "emsg": [{n: int(er[s]) for n, s in EMSG.items()} for er in emsg[k] if er[EMSG["offset"]] >= 0]}
            if plain < 0:
                r["error"] = ValueError(ERR_PADDING)
            _attach(r, g, k, job, sinfo[k].tolist())
            if g.cbinfo is not None:
                view = cbcs_view if g.scheme == "cbcs" else cenc_view
                r[g.scheme] = MappingProxyType(view(_np(g.cbinfo)[k]))
            yield r


class _Packed:
    """Packed audio (docs/PACKEDAUDIO.md): one ``packed_audio_batch`` per group, whose views stand in
    for the demux and the index, the remux of :meth:`MediaPipeline._launch_remux` over them, and
    results of the MPEG-TS shape with ``packed_audio``."""

    name, captions, remux = "aac", False, True

    @staticmethod
    def demux(jobs, rows, buf, offs, lens, caps):
        from ..ops import packedaudio as _pa

        pa = _pa.packed_audio_batch(buf, offs, lens, caps=caps)
        return _Group(rows, pa.as_demux(), hlens=_to_host(lens), hinfo=_to_host(pa.info), ix=pa.as_index(),
                      sinfo=_to_host(pa.sinfo), painfo=_to_host(pa.painfo))

    @staticmethod
    def rows(g, jobs):
        from ..ops.packedaudio import FATAL, PAINFO, PASTATUS

        res = g.res
        rl, srows, prows, hlens = _np(g.hinfo).tolist(), _np(g.sinfo).tolist(), _np(g.painfo).tolist(), _np(g.hlens)
        for k, (i, base) in enumerate(zip(g.rows.tolist(), res.es_offs.tolist())):
            pa = prows[k]
            r = _ts_result(res, res.es, k, rl[k], base, int(hlens[k]))
            r["packed_audio"] = MappingProxyType({name: pa[slot] for name, slot in PAINFO.items()})
            if "error" not in r and pa[PAINFO["status"]] & FATAL:
                names = [name for name, bit in PASTATUS.items() if pa[PAINFO["status"]] & FATAL & bit]
                r["error"] = ValueError("packed audio: " + ", ".join(names))
            _attach(r, g, k, jobs[i], srows[k])
            yield r


def _any(mask: Optional[np.ndarray], rows: np.ndarray) -> bool:
    """A row of ``rows`` is set in ``mask`` (``None``: nobody asked)."""
    return mask is not None and bool(mask[rows].any())


def _mask(n: int, idx) -> Optional[np.ndarray]:
    """bool[n] with ``idx`` set (None when ``idx`` is empty)."""
    if not len(idx):
        return None
    m = np.zeros(n, dtype=bool)
    m[np.asarray(idx, dtype=np.int64)] = True
    return m


_UNSUPPORTED_VIDEO = 16  # ops.codecconfig.CSTATUS["unsupported_video"]
_VB, _AB, _IB = _ts.INFO["video_bytes"], _ts.INFO["audio_bytes"], _ts.INFO["id3_bytes"]
_AO, _IO = _ts.INFO["audio_es_offset"], _ts.INFO["id3_es_offset"]


class _Result(dict):
    """One fragment's transmux result: ``status``, ``info``, ``plain_bytes``, ``demux``,
    ``index`` (and ``error``) stored; ``video`` / ``audio`` / ``id3`` ES views of the batch's
    ES buffer made on first access."""

    __slots__ = ("_es",)

    def __missing__(self, key):
        if key not in ("video", "audio", "id3"):
            raise KeyError(key)
        es, base, vb, ab, ib, ao, io = self._es
        v = es.narrow(0, base, vb)
        a = es.narrow(0, base + ao, ab)
        i = es.narrow(0, base + io, ib)
        self["video"], self["audio"], self["id3"] = v, a, i
        return self[key]


class InfoRow:
    """Read-only ``{name: value}`` view of one demux ``info`` row (names of
    :data:`ops.tsdemux.INFO`), sharing one key->slot schema instead of a dict per fragment."""

    __slots__ = ("_row",)
    _SLOTS = _ts.INFO

    def __init__(self, row) -> None:
        self._row = row

    def __getitem__(self, name: str) -> int:
        return self._row[self._SLOTS[name]]

    def get(self, name: str, default=None):
        slot = self._SLOTS.get(name)
        return default if slot is None else self._row[slot]

    def keys(self):
        return self._SLOTS.keys()

    def items(self):
        return ((k, self._row[v]) for k, v in self._SLOTS.items())

    def __contains__(self, name: str) -> bool:
        return name in self._SLOTS

    def __iter__(self):
        return iter(self._SLOTS)

    def __len__(self) -> int:
        return len(self._SLOTS)

    def to_dict(self):
        return dict(self.items())

    def __repr__(self) -> str:
        return f"InfoRow({self.to_dict()})"


class _View:
    """The read-only mapping protocol of the result views below, from ``keys()`` and ``__getitem__``."""

    __slots__ = ()

    def get(self, name: str, default=None):
        try:
            return self[name]
        except KeyError:
            return default

    def items(self):
        return ((k, self[k]) for k in self.keys())

    def __contains__(self, name) -> bool:
        return name in self.keys()

    def __iter__(self):
        return iter(self.keys())

    def __len__(self) -> int:
        return len(self.keys())


class Samples(_View):
    """Read-only mapping of one fragment's sample index (``TransmuxJob.index``): the ``sinfo``
    fields by name (:data:`ops.esindex.SINFO`), ``independent`` (access unit 0 holds a
    keyframe), and ``nal`` / ``au`` / ``aframes``: the fragment's rows of the batch's device
    tables, viewed on first access."""

    __slots__ = ("_row", "_ix", "_k")
    _TABLES = ("nal", "au", "aframes")

    def __init__(self, row, ix, k: int) -> None:
        self._row = row
        self._ix = ix
        self._k = k

    def __getitem__(self, name: str):
        from ..ops.esindex import SINFO

        slot = SINFO.get(name)
        if slot is not None:
            return self._row[slot]
        if name == "independent":
            return self._row[SINFO["first_keyframe_au"]] == 0
        if name in self._TABLES:
            return getattr(self._ix, name)[self._k]
        raise KeyError(name)

    def keys(self):
        from ..ops.esindex import SINFO

        return list(SINFO) + ["independent", *self._TABLES]

    def __repr__(self) -> str:
        fields = {k: self[k] for k in self.keys() if k not in self._TABLES}
        return f"Samples({fields})"


class CaptionData(_View):
    """Read-only mapping of one fragment's caption data (``TransmuxJob.captions``): the ``ccinfo``
    fields by name (:data:`ops.captions.CCINFO`), ``samples`` / ``pts`` / ``bytes`` / ``cc608`` (the
    fragment's rows of the batch's device tables, viewed on first access) and ``host()``: the
    host view of :func:`ops.captions.segment_view` (``samples`` as hls.js's user-data samples and
    ``field1`` / ``field2``, in presentation order), which syncs and is built on first call."""

    __slots__ = ("_g", "_k", "_host")
    _TABLES = {"samples": "ccsamples", "pts": "ccpts", "bytes": "ccbytes", "cc608": "cc608"}

    def __init__(self, group, k: int) -> None:
        self._g = group
        self._k = k
        self._host: Any = None

    def host(self) -> Dict[str, Any]:
        if self._host is None:
            self._host = self._g.cc.segment(self._k)
        return self._host

    def __getitem__(self, name: str):
        from ..ops.captions import CCINFO

        slot = CCINFO.get(name)
        if slot is not None:
            return int(_np(self._g.ccinfo)[self._k, slot])
        if name in self._TABLES:
            return getattr(self._g.cc, self._TABLES[name])[self._k]
        if name == "host":
            return self.host
        raise KeyError(name)

    def keys(self):
        from ..ops.captions import CCINFO

        return [*CCINFO, *self._TABLES, "host"]

    def __repr__(self) -> str:
        from ..ops.captions import CCINFO

        return f"CaptionData({ {k: self[k] for k in CCINFO} })"


class Fmp4Track(_View):
    """Read-only mapping of one remuxed track of a fragment: ``mdat`` (a device view of the whole
    box, header included), ``samples`` (the filled device rows of the track's sample table),
    ``nb`` (samples), ``base`` / ``duration`` / ``timescale`` (the fragment's decode time and
    length in the track's units) and ``moof(sequence_number)`` (host bytes, built on first call);
    from the fragment's codec configuration ``init`` (the track's init segment as host bytes, built
    on first access, ``None`` when the configuration cannot describe the track), ``codec`` (the RFC
    6381 string, ``None`` like ``init``), ``container`` and ``width`` / ``height`` (video) or
    ``channelCount`` / ``samplerate`` (audio).  The video track of an HEVC fragment (``config`` says
    ``unsupported_video`` and ``hevc`` has no disqualifying bit) takes the four from ``hevc``.
    For a job that asked for its moof boxes (``TransmuxJob.fragment``) also ``moof_view`` (a device
    view of the track's ``moof``, which ends where ``mdat`` starts), ``fragment`` (one device view
    over both) and ``tfdt`` (the box's decode time, in the track's units)."""

    __slots__ = ("_f", "_video", "_moofs", "_init")
    _KEYS = ("mdat", "samples", "nb", "base", "duration", "timescale", "moof", "init", "codec", "container")
    _UNBUILT = object()

    def __init__(self, f: "Fmp4", video: bool) -> None:
        self._f = f
        self._video = video
        self._moofs: Dict[int, bytes] = {}
        self._init: Any = self._UNBUILT

    def _config_key(self, name: str):
        from . import fmp4 as _fmp4

        cfg = self._f["config"]
        if name == "container":
            return "video/mp4" if self._video else "audio/mp4"
        dolby = None if self._video else self._f._dolby()
        if dolby is not None:  # an AC-3 / E-AC-3 track: the four come from its ac3info row
            if name == "init":
                if self._init is self._UNBUILT:
                    self._init = _fmp4.ac3_audio_init(dolby)
                return self._init
            if name == "codec":
                return _fmp4.ac3_audio_codec(dolby)
            return dolby["channels" if name == "channelCount" else "sample_rate"]
        mpa = None if self._video else self._f._mpa()
        if mpa is not None:  # an MPEG audio track: the four come from its mpainfo row
            if name == "init":
                if self._init is self._UNBUILT:
                    self._init = _fmp4.mpeg_audio_init(mpa)
                return self._init
            if name == "codec":
                return _fmp4.mpeg_audio_codec(mpa)
            return mpa["channels" if name == "channelCount" else "sample_rate"]
        if self._video and cfg["status"] & _UNSUPPORTED_VIDEO:
            hevc = self._f["hevc"]
            if not hevc["status"] & _fmp4.HEVC_DISQUALIFIED:
                if name == "init":
                    if self._init is self._UNBUILT:
                        self._init = _fmp4.hevc_init(hevc)
                    return self._init
                return _fmp4.hevc_codec(hevc) if name == "codec" else hevc[name]  # width / height
        if name == "init":
            if self._init is self._UNBUILT:
                self._init = _fmp4.video_init(cfg) if self._video else _fmp4.audio_init(cfg)
            return self._init
        if name == "codec":
            if cfg["status"] & (_fmp4.VIDEO_DISQUALIFIED if self._video else _fmp4.AUDIO_DISQUALIFIED):
                return None
            return _fmp4.video_codec(cfg) if self._video else _fmp4.audio_codec(cfg)
        if name == "channelCount":
            return _fmp4.audio_channels(cfg)
        if name == "samplerate":
            return _fmp4.audio_sample_rate(cfg)
        return cfg[name]  # width / height

    def _host_rows(self) -> np.ndarray:
        f = self._f
        if self._video:
            return _np(f._g.vsamples)[f._k, :self["nb"]]
        rows = _np(f._g.asamples)[f._k]
        return rows[:self["nb"]]

    def moof(self, sequence_number: int) -> bytes:
        from . import fmp4 as _fmp4

        data = self._moofs.get(sequence_number)
        if data is None:
            f = self._f
            if self._video:
                data = _fmp4.video_moof(sequence_number, f._rinfo("video_base_dts"), self._host_rows())
            else:
                data = _fmp4.audio_moof(sequence_number, f._rinfo("audio_base_pts"), f._audio_rate(), self._host_rows(),
                                        f._frame_samples())
            self._moofs[sequence_number] = data
        return data

    def __getitem__(self, name: str):
        from . import fmp4 as _fmp4

        f = self._f
        rx = f._g.rx
        if name == "nb":
            if self._video:
                return f._rinfo("n_vsamples")
            return int((_np(f._g.asamples)[f._k, :, 0] >= 0).sum())
        if name == "mdat":
            o = int(rx.out_offs[f._k]) + (0 if self._video else f._rinfo("audio_box_offset"))
            return rx.out.narrow(0, o, 8 + f._rinfo("video_payload_bytes" if self._video else "audio_payload_bytes"))
        if name == "samples":
            return (rx.vsamples if self._video else rx.asamples)[f._k, :self["nb"]]
        if name == "timescale":
            return _fmp4.VIDEO_TIMESCALE if self._video else f._audio_rate()
        if name == "base":
            if self._video:
                return max(f._rinfo("video_base_dts"), 0)
            return _fmp4.audio_base(f._rinfo("audio_base_pts"), f._audio_rate())
        if name == "duration":
            if self._video:
                return int(self._host_rows()[:, 2].sum(dtype=np.int64))
            return f._frame_samples() * self["nb"]
        if name == "moof":
            return self.moof
        if name in ("fragment", "moof_view", "tfdt") and f._fragment:
            if name == "tfdt":
                return f._finfo("video_tfdt" if self._video else "audio_tfdt")
            moof = f._finfo("video_moof_bytes" if self._video else "audio_moof_bytes")
            end = int(rx.out_offs[f._k]) + (0 if self._video else f._rinfo("audio_box_offset"))
            if name == "moof_view":
                return rx.out.narrow(0, end - moof, moof)
            return rx.out.narrow(0, end - moof, moof + 8 + f._rinfo("video_payload_bytes" if self._video
                                                                     else "audio_payload_bytes"))
        if name in ("init", "codec", "container") or name in (("width", "height") if self._video
                                                              else ("channelCount", "samplerate")):
            return self._config_key(name)
        raise KeyError(name)

    def keys(self):
        return list(self._KEYS) + (["width", "height"] if self._video else ["channelCount", "samplerate"]) \
            + (["fragment", "moof_view", "tfdt"] if self._f._fragment else [])

    def __repr__(self) -> str:
        return f"Fmp4Track({'video' if self._video else 'audio'}, nb={self['nb']})"


class Fmp4(_View):
    """Read-only mapping of one fragment's remux (``TransmuxJob.remux``): ``video`` and ``audio``
    (:class:`Fmp4Track`), the ``rinfo`` fields by name (:data:`ops.remux.RINFO`) and ``config``: the
    fragment's codec configuration, a read-only mapping of the ``cinfo`` fields by name
    (:data:`ops.codecconfig.CINFO`) plus ``sps`` / ``pps`` as bytes, and ``hevc``: the same of the
    ``hinfo`` fields (:data:`ops.hevcconfig.HINFO`) plus ``vps`` / ``sps`` / ``pps``, and
    ``mpeg_audio``: the ``mpainfo`` fields by name (:data:`ops.mpegaudio.MPAINFO`); where that has a
    config (neither ``not_mpeg_audio`` nor ``no_audio_config``) the audio track is an MPEG audio
    track and takes its time scale, frame length, init segment and codec from there.  ``ac3_audio``
    is the same of the ``ac3info`` fields (:data:`ops.ac3audio.AC3INFO`) for an AC-3 / E-AC-3 track; it is
    listed among the keys of a segment whose audio type is Dolby audio.  For a job that
    asked for its moof boxes also ``time_base``: the 90 kHz base its ``tfdt`` values are relative to."""

    __slots__ = ("_g", "_k", "_rate", "_tracks", "_config", "_hevc", "_fragment", "_mpeg", "_ac3")

    def __init__(self, group, k: int, sinfo_row, fragment: bool = False) -> None:
        from ..ops.esindex import SINFO

        self._g = group  # the fragment's _Group: its Remuxed and the three host tables
        self._k = k
        self._fragment = fragment  # the job asked for its moof boxes: ``time_base``, and three more keys per track
        self._rate = sinfo_row[SINFO["audio_sample_rate"]]
        self._tracks: Dict[str, Fmp4Track] = {}
        self._config: Any = None
        self._hevc: Any = None
        self._mpeg: Any = None
        self._ac3: Any = None

    def _mpa(self):
        """The ``mpeg_audio`` mapping where it has a config, else ``None``."""
        from ..ops.mpegaudio import NO_CONFIG

        m = self["mpeg_audio"]
        return None if m["status"] & NO_CONFIG else m

    def _dolby(self):
        """The ``ac3_audio`` mapping where it has a config, else ``None``."""
        from ..ops.ac3audio import NO_CONFIG

        m = self["ac3_audio"]
        return None if m["status"] & NO_CONFIG else m

    def _frames(self):
        """The mapping of the audio track's frame codec (MPEG audio or Dolby audio) where one has a
        config, else ``None``: an ADTS track."""
        m = self._mpa()
        return m if m is not None else self._dolby()

    def _frame_samples(self) -> int:
        from . import fmp4 as _fmp4

        m = self._frames()
        return _fmp4.AAC_FRAME_SAMPLES if m is None else m["frame_samples"]

    def _audio_rate(self) -> int:
        m = self._frames()
        return self._rate if m is None else m["sample_rate"]

    def _rinfo(self, name: str) -> int:
        from ..ops.remux import RINFO

        return int(_np(self._g.rinfo)[self._k, RINFO[name]])

    def _finfo(self, name: str) -> int:
        from ..ops.fragment import FINFO

        return int(_np(self._g.finfo)[self._k, FINFO[name]])

    def __getitem__(self, name: str):
        from ..ops.remux import RINFO

        if name in ("video", "audio"):
            t = self._tracks.get(name)
            if t is None:
                t = self._tracks[name] = Fmp4Track(self, name == "video")
            return t
        if name in RINFO:
            return self._rinfo(name)
        if name == "time_base" and self._fragment:
            return self._finfo("time_base")
        if name == "config":
            if self._config is None:
                from ..ops.codecconfig import segment_view

                g, k = self._g, self._k
                self._config = MappingProxyType(segment_view(_np(g.cinfo)[k], _np(g.ps)[k]))
            return self._config
        if name == "hevc":
            if self._hevc is None:
                from ..ops.hevcconfig import segment_view

                g, k = self._g, self._k
                self._hevc = MappingProxyType(segment_view(_np(g.hvinfo)[k], _np(g.hps)[k]))
            return self._hevc
        if name == "mpeg_audio":
            if self._mpeg is None:
                from ..ops.mpegaudio import MPAINFO

                row = _np(self._g.mpainfo)[self._k]
                self._mpeg = MappingProxyType({k: int(row[v]) for k, v in MPAINFO.items()})
            return self._mpeg
        if name == "ac3_audio":
            if self._ac3 is None:
                from ..ops.ac3audio import AC3INFO

                row = _np(self._g.ac3info)[self._k]
                self._ac3 = MappingProxyType({k: int(row[v]) for k, v in AC3INFO.items()})
            return self._ac3
        raise KeyError(name)

    def keys(self):
        from ..ops.remux import RINFO

        from ..ops.ac3audio import AC3STATUS

        dolby = [] if self["ac3_audio"]["status"] & AC3STATUS["not_dolby_audio"] else ["ac3_audio"]
        return ["video", "audio", *RINFO, "config", "hevc", "mpeg_audio"] + dolby \
            + (["time_base"] if self._fragment else [])

    def __repr__(self) -> str:
        views = ("video", "audio", "config", "hevc", "mpeg_audio", "ac3_audio")
        return f"Fmp4({ {k: self[k] for k in self.keys() if k not in views} })"


class Mp4TrackView(_View):
    """Read-only mapping of one track of a fragmented-MP4 fragment: ``nb`` (samples), ``base`` (decode
    time of its first sample-bearing ``traf``), ``duration``, ``min_pts`` / ``max_pts``, ``first_sync``,
    ``first_pts`` / ``last_pts`` (all in the track's ``timescale``), ``id`` and ``codec`` from the init
    segment, and ``samples`` / ``pes``: the fragment's rows of the batch's device tables
    (``msamples``: size, duration, cts, flags; ``pes``: offset in ``data``, pts, dts), viewed on
    first access."""

    __slots__ = ("_md", "_k", "_t", "_row", "_info", "_init")
    _FIELDS = {"nb": "n_samples", "base": "base_time", "duration": "duration", "min_pts": "min_pts",
               "max_pts": "max_pts", "first_sync": "first_sync"}

    def __init__(self, md, k: int, t: int, row, info, init) -> None:
        self._md, self._k, self._t, self._row, self._info, self._init = md, k, t, row, info, init

    def __getitem__(self, name: str):
        from ..ops.mp4demux import MINFO_TRACK, MINFO_TRACK0, MINFO_TRACK_WORDS

        kind = ("video", "audio")[self._t]
        if name in self._FIELDS:
            return self._row[MINFO_TRACK0 + MINFO_TRACK_WORDS * self._t + MINFO_TRACK[self._FIELDS[name]]]
        if name == "timescale":
            return int(self._init.timescale.get(kind, 0))
        if name in ("first_pts", "last_pts"):
            return int(self._info[_ts.INFO[f"{kind}_{name}"]])
        if name == "id":
            track = getattr(self._init, kind)
            return track.track_id if track is not None else -1
        if name == "codec":
            return getattr(self._init, f"{kind}_codec")
        if name == "samples":
            return self._md.msamples[self._k, self._t, :min(self["nb"], self._md.msamples.shape[2])]
        if name == "pes":
            return self._md.pes[self._k, self._t, :min(self["nb"], self._md.pes.shape[2])]
        raise KeyError(name)

    def keys(self):
        return [*self._FIELDS, "timescale", "first_pts", "last_pts", "id", "codec", "samples", "pes"]

    def __repr__(self) -> str:
        return f"Mp4TrackView({ {k: self[k] for k in self.keys() if k not in ('samples', 'pes')} })"


@dataclass(eq=False)
class _Group:
    """One demux group of a batch (its encrypted rows, or its clear ones) and what was run on it."""
    rows: np.ndarray  # rows of the batch, in the group's order
    res: Any  # the group's DemuxResult, on the device
    hinfo: Any  # its info rows and ...
    hlens: Any  # ... plaintext lengths on the host (pinned: readable after the batch's event)
    ix: Any = None  # EsIndex, when a job of the group asked for it, with ...
    sinfo: Any = None  # ... its sinfo rows on the host
    sa: Any = None  # SampleAes, when a job of the group asked for it, with ...
    sainfo: Any = None  # ... its sainfo rows on the host
    cc: Any = None  # Captions, when a job of the group asked for it, with ...
    ccinfo: Any = None  # ... its ccinfo rows on the host
    rx: Any = None  # Remuxed, when a job of the group asked for it, with ...
    rinfo: Any = None  # ... its three tables on the host
    vsamples: Any = None
    asamples: Any = None
    fr: Any = None  # Fragments, when a job of the group asked for its moof boxes, with ...
    finfo: Any = None  # ... its finfo rows on the host
    cfg: Any = None  # CodecConfig, behind the remux, with ...
    cinfo: Any = None  # ... its two tensors on the host
    ps: Any = None
    hcfg: Any = None  # HevcConfig, behind the codec configuration, with ...
    hvinfo: Any = None  # ... its two tensors on the host
    hps: Any = None
    ma: Any = None  # MpegAudio, directly behind the remux, with ...
    mpainfo: Any = None  # ... its mpainfo rows on the host
    da: Any = None  # Ac3Audio, behind the MPEG audio op, with ...
    ac3info: Any = None  # ... its ac3info rows on the host
    painfo: Any = None  # the painfo rows of a packed-audio group on the host
    md: Any = None  # the Mp4Demux of a fragmented-MP4 group (of a cbcs or cenc group: over the decrypted copy) ...
    minfo: Any = None  # ... with its minfo rows and emsg table on the host; res / ix are its views
    emsg: Any = None
    cbinfo: Any = None  # the cinfo rows of a cbcs or cenc group on the host
    scheme: str = ""    # "cbcs" / "cenc" where cbinfo is set


@dataclass(eq=False)
class _Aside:
    """The jobs of a batch that were set aside as one container, and their launch."""
    kind: Any  # _Mp4 / _Packed
    jobs: List[TransmuxJob]
    groups: List[_Group]
    event: Any
    error: Optional[BaseException]
    rejected: Any  # jobs whose encrypted payload is not whole AES blocks
    start: Any = None  # (no timing event: a batch's device time is its MPEG-TS core's)


@dataclass(eq=False)
class _Batch:
    jobs: List[TransmuxJob]
    groups: List[_Group] = field(default_factory=list)
    event: Any = None
    error: Optional[BaseException] = None
    keep: Any = None  # device/pinned buffers the batch's in-flight work uses
    tag: Any = None  # launch_columns: the caller's columns, handed back by complete_columns
    n: int = 0  # fragments in the batch
    start: Any = None  # timing event recorded before the batch's first launch
    verify: Any = None  # [(fragment indices, ok flags (pinned uint8 / bool))] of expect-CRC checks
    expect_mask: Any = None  # bool[n]: fragments that asked for a CRC check (unchecked ones fail)
    aside: Any = ()  # [_Aside]: the batch's fragmented-MP4 jobs, then its packed-audio jobs, which took their own path

    # the groups as the benchmark's output dump reads them: derived, nothing is stored twice
    @property
    def infos(self):
        return [(g.rows, g.res, g.res.es_offs, g.hlens) for g in self.groups]

    @property
    def host(self):
        return [(g.hinfo, g.hlens) for g in self.groups]


_local = threading.local()


def pipeline_for(device: torch.device, loop=None) -> MediaPipeline:
    """The calling thread's pipeline for ``device``."""
    cache = getattr(_local, "pipes", None)
    if cache is None:
        cache = {}
        _local.pipes = cache
    loop = loop or get_event_loop()
    key = (str(device), id(loop))
    p = cache.get(key)
    if p is None:
        p = MediaPipeline(device, loop)
        cache[key] = p
    return p


def default_transmux_device() -> torch.device:
    return torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cpu")
