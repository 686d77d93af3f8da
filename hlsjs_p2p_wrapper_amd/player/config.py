"""hls.js-style configuration object.

A plain mapping with attribute access, so both ``hls.config.maxBufferLength`` (hls.js
style, mutated by the player bridge at ``lib/integration/player-interface.js:63-66``) and
``config["fLoader"]`` work.  ``None`` plays the role of JavaScript ``undefined``.

Defaults follow hls.js 0.5/0.6 (the versions the reference supports, ``README.md:6-9``)
for every key the engine implements, plus the MI355X-engine extensions at the bottom.
"""
from __future__ import annotations

import math
from typing import Any, Dict, Mapping, Optional


class HlsConfig(dict):
    def __getattr__(self, name: str) -> Any:
        try:
            return self[name]
        except KeyError:
            if name.startswith("__"):
                raise AttributeError(name)
            return None

    def __setattr__(self, name: str, value: Any) -> None:
        self[name] = value

    def __delattr__(self, name: str) -> None:
        self.pop(name, None)

    def copy(self) -> "HlsConfig":
        return HlsConfig(self)


def _default_config() -> Dict[str, Any]:
    from .abr import AbrController
    from .loader import XhrLoader
    from .controllers import StreamController

    return {
        "autoStartLoad": True,
        "startPosition": -1,
        "debug": False,
        "capLevelToPlayerSize": False,
        "maxBufferLength": 30,
        "maxBufferSize": 60 * 1000 * 1000,
        "maxBufferHole": 0.5,
        "maxSeekHole": 2,
        "seekHoleNudgeDuration": 0.01,
        "maxFragLookUpTolerance": 0.2,
        "liveSyncDurationCount": 3,
        "liveMaxLatencyDurationCount": math.inf,
        "liveSyncDuration": None,
        "liveMaxLatencyDuration": None,
        "maxMaxBufferLength": 600,
        "enableWorker": True,
        "enableSoftwareAES": True,
        "manifestLoadingTimeOut": 10000,
        "manifestLoadingMaxRetry": 1,
        "manifestLoadingRetryDelay": 1000,
        "levelLoadingTimeOut": 10000,
        "levelLoadingMaxRetry": 4,
        "levelLoadingRetryDelay": 1000,
        "fragLoadingTimeOut": 20000,
        "fragLoadingMaxRetry": 6,
        "fragLoadingRetryDelay": 1000,
        "fragLoadingLoopThreshold": 3,
        "startFragPrefetch": False,
        "appendErrorMaxRetry": 3,
        "loader": XhrLoader,
        "fLoader": None,
        "pLoader": None,
        "xhrSetup": None,
        "abrController": AbrController,
        "streamController": StreamController,
        "abrEwmaFastLive": 5.0,
        "abrEwmaSlowLive": 9.0,
        "abrEwmaFastVoD": 4.0,
        "abrEwmaSlowVoD": 15.0,
        "abrEwmaDefaultEstimate": 5e5,
        "abrBandWidthFactor": 0.8,
        "abrBandWidthUpFactor": 0.7,
        "minAutoBitrate": 0,
        # --- MI355X engine extensions ------------------------------------------------
        # fragments loaded concurrently (hls.js loads one at a time: 1 keeps parity;
        # serving/throughput deployments raise it so one exchange round moves many)
        "maxFragLoadsInFlight": 1,
        # where decrypt/demux run: "auto" (the media pipeline's device), "cpu", "cuda:N"
        "transmuxDevice": "auto",
        # stream-controller tick period (hls.js uses 100 ms)
        "tickInterval": 100,
        # keep demuxed ES tensors referenced by the media element (False: account only)
        "retainMediaData": False,
        # index NAL units, access units and ADTS frames of every fragment on the transmux
        # device (docs/ESINDEX.md): FRAG_PARSING_DATA gains "samples", FRAG_PARSED "independent"
        "indexSamples": False,
        # remux every fragment to fragmented MP4 on the transmux device (docs/REMUX.md; implies the
        # index): FRAG_PARSING_DATA carries the moof in "data1", the mdat device view in "data2",
        # "startDTS" / "endDTS" and the sample count in "nb"; FRAG_PARSING_INIT_SEGMENT carries each
        # track's init segment, codec and container (docs/INITSEGMENT.md)
        "remuxFmp4": False,
        # write each track's moof on the transmux device too, directly in front of its mdat
        # (docs/FRAGMENT.md; implies remuxFmp4): FRAG_PARSING_DATA carries the moof as a device view
        # in "data1", adjacent to the mdat view in "data2", and "fragment", one view over both; the
        # tfdt, "startDTS" and "endDTS" are on the playlist's timeline (one initPTS per discontinuity
        # counter, 33-bit rollovers unwrapped)
        "fmp4Fragments": False,
        # extract the CEA-608/708 caption data of every fragment's SEI NAL units on the transmux
        # device (docs/CAPTIONS.md; implies the index) and emit it on FRAG_PARSING_USERDATA; hls.js's
        # name, off by default here like every device feature
        "enableCEA708Captions": False,
        # packed audio (docs/PACKEDAUDIO.md): a fragment of ID3v2 tags in front of raw ADTS frames,
        # demuxed on the transmux device with the events of an MPEG-TS fragment.  "auto": a fragment
        # without #EXT-X-MAP whose URL path ends in ".aac" (query dropped, any letter case);
        # True: every fragment without a map; False: none (such a fragment fails in the TS demux)
        "packedAudio": "auto",
    }


_DEFAULTS: Optional[Dict[str, Any]] = None


def default_config() -> HlsConfig:
    global _DEFAULTS
    if _DEFAULTS is None:
        _DEFAULTS = _default_config()
    return HlsConfig(_DEFAULTS)


def merge_config(user: Optional[Mapping[str, Any]]) -> HlsConfig:
    """hls.js constructor semantics: user keys override defaults (``undefined`` skipped)."""
    cfg = default_config()
    if user:
        for k, v in user.items():
            if v is not None:
                cfg[k] = v
    return cfg
