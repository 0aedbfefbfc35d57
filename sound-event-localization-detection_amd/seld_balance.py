"""Class-balanced window sampling of the device feed: weights and the epoch's order.  Host-side numpy
only; the per-window class statistics come from ``SELDDataset.window_class_counts`` (csrc/balance.hip).

``counts`` is int32 [N, 16]: column c < 14 = frames of the window in which class c is active somewhere on the grid, column 14 =
frames with any class active, column 15 = frames of the window inside the timeline.

    presence     class c is PRESENT in window w when counts[w, c] >= BALANCE_MIN_FRAMES; a window with a present class is
                 ACTIVE, every other one SILENT
    rarity       n_c = windows in which c is present
    active w     r_w = max over the present c of n_c ** -BALANCE_POWER        (n_c ** -beta: ``math.pow`` of a Python float)
    silent w     all the same weight s, chosen so that their expected share of the draws is BALANCE_SILENT_SHARE:
                 s = (share * A) / ((1 - share) * |S|),  A = the exactly rounded sum (``math.fsum``) of the active weights,
                 share = |S| / N for None (their natural share); with no silent window the share is ignored
    quantised    k_w = floor(weight_w / max weight * 2^32 + 0.5) as int64, at least 1 for a positive weight

From the int64 table ``k`` on everything is integer arithmetic: the epoch's order is
``searchsorted(cumsum(k), default_rng([seed, epoch, 0, 3]).integers(0, sum k, N), side="right")`` -- N draws with
replacement, a pure function of (counts, settings, seed, epoch), the same on every rank and in a resumed run.
"""
from __future__ import annotations

import math
import zlib

import numpy as np

COLUMNS = 16                      # SELD_BALANCE_COLUMNS
MAX_CLASSES = 14                  # SELD_BALANCE_MAX_CLASSES
ANY, FRAMES = 14, 15              # the two columns behind the classes
SCALE = float(1 << 32)            # the largest weight's k
STREAM = (0, 3)                   # tail of the draw's generator key [seed, epoch, 0, 3]: none of seld_augment's streams


def settings(cfg) -> dict:
    """The sampling switches of a Config as a plain dict (missing attributes = defaults, the switch off)."""
    share = getattr(cfg, "BALANCE_SILENT_SHARE", None)
    return {"enabled": bool(getattr(cfg, "BALANCED_SAMPLING", False)),
            "power": float(getattr(cfg, "BALANCE_POWER", 1.0)),
            "silent_share": None if share is None else float(share),
            "min_frames": getattr(cfg, "BALANCE_MIN_FRAMES", 5)}


def check_settings(s) -> dict:
    """Raise ValueError for values outside their range; ``s``: a Config or the dict of ``settings``."""
    if not isinstance(s, dict):
        s = settings(s)
    if not 0.0 <= s["power"] <= 1.0:                     # a NaN fails both comparisons
        raise ValueError(f"BALANCE_POWER must be in [0, 1], got {s['power']}")
    if s["silent_share"] is not None and not 0.0 <= s["silent_share"] < 1.0:
        raise ValueError(f"BALANCE_SILENT_SHARE must be None or in [0, 1), got {s['silent_share']}")
    frames = s["min_frames"]
    if isinstance(frames, bool) or not isinstance(frames, (int, np.integer)) or frames < 1:
        raise ValueError(f"BALANCE_MIN_FRAMES must be an integer >= 1, got {frames!r}")
    return s


def _table(counts) -> np.ndarray:
    counts = np.asarray(counts)
    if counts.ndim != 2 or counts.shape[1] != COLUMNS or not np.issubdtype(counts.dtype, np.integer):
        raise ValueError(f"counts must be an integer [N, {COLUMNS}] table (SELDDataset.window_class_counts)")
    return counts


def presence(counts, min_frames: int) -> np.ndarray:
    """bool [N, 14]: class c is present in window w."""
    return _table(counts)[:, :MAX_CLASSES] >= int(min_frames)


def weights(counts, s) -> np.ndarray:
    """float64 [N]: the windows' draw weights before quantisation (module docstring)."""
    s = check_settings(s)
    present = presence(counts, s["min_frames"])
    active = present.any(axis=1)
    n_windows, n_active = len(active), int(active.sum())
    if n_active == 0:
        raise ValueError("balanced sampling: no window holds a class for BALANCE_MIN_FRAMES frames, so there is nothing to "
                         "balance (an unlabelled dataset, or BALANCE_MIN_FRAMES above every event's length)")
    n_c = present.sum(axis=0)
    rarity = np.array([math.pow(float(n), -s["power"]) if n else 0.0 for n in n_c], dtype=np.float64)
    w = np.where(present, rarity[None, :], 0.0).max(axis=1)
    n_silent = n_windows - n_active
    if n_silent:
        share = n_silent / n_windows if s["silent_share"] is None else s["silent_share"]
        w[~active] = (share * math.fsum(w[active].tolist())) / ((1.0 - share) * n_silent)
    return w


def quantise(w) -> np.ndarray:
    """int64 [N]: k_w = floor(w / max w * 2^32 + 0.5), at least 1 for a positive weight, 0 for weight 0."""
    w = np.asarray(w, dtype=np.float64)
    if w.ndim != 1 or not (np.isfinite(w).all() and (w >= 0).all() and w.max(initial=0.0) > 0):
        raise ValueError("quantise: weights must be finite, not negative and not all zero")
    k = np.floor(w / w.max() * SCALE + 0.5).astype(np.int64)
    return np.where(w > 0, np.maximum(k, 1), 0)


def window_weights(counts, s) -> np.ndarray:
    """The int64 [N] table ``k`` an epoch's order is drawn from."""
    return quantise(weights(counts, s))


def order(k, seed: int, epoch: int) -> np.ndarray:
    """int64 [N]: the window indices of ``epoch`` in the order they are trained on -- N = len(k) draws with replacement,
    window w with probability k_w / sum k.  Shard it with ``trainer.shard_indices``."""
    k = np.asarray(k, dtype=np.int64)
    cum = np.cumsum(k, dtype=np.int64)
    if k.ndim != 1 or len(k) == 0 or (k < 0).any() or cum[-1] <= 0:
        raise ValueError("order: k must be a non-empty table of weights >= 0 with a positive sum")
    u = np.random.default_rng([int(seed), int(epoch), *STREAM]).integers(0, int(cum[-1]), size=len(k), dtype=np.int64)
    return np.searchsorted(cum, u, side="right").astype(np.int64)


def exposure(counts, k, s) -> dict:
    """What the weights do, from the table alone: per class the natural share n_c / N of the windows that hold it and the
    expected share under the weights (sum of k over those windows / sum k), and the silent windows' share before and after.
    A window with two classes counts for both; mix partners (AUGMENT_MIX_PROB) are drawn uniformly and are not counted."""
    s = check_settings(s)
    present = presence(counts, s["min_frames"])
    k = np.asarray(k, dtype=np.int64)
    if k.shape != (len(present),):
        raise ValueError("exposure: k must hold one weight per row of counts")
    total = int(k.sum())
    silent = ~present.any(axis=1)
    return {"windows": len(k),
            "class_windows": present.sum(axis=0).astype(np.int64),
            "natural": present.sum(axis=0) / len(k),
            "expected": np.array([int(k[present[:, c]].sum()) / total for c in range(MAX_CLASSES)], dtype=np.float64),
            "silent_natural": float(silent.sum()) / len(k),
            "silent_expected": int(k[silent].sum()) / total}


def describe(e, num_classes: int = MAX_CLASSES) -> str:
    """One log line of an ``exposure`` report."""
    per_class = ", ".join(f"{c}: {100 * e['natural'][c]:.1f} -> {100 * e['expected'][c]:.1f}"
                          for c in range(min(int(num_classes), MAX_CLASSES)) if e["class_windows"][c])
    return (f"{e['windows']} windows, silent {100 * e['silent_natural']:.2f} % -> {100 * e['silent_expected']:.2f} % of the "
            f"draws; windows holding class c, % natural -> % expected: {per_class}")


def table_crc(k) -> int:
    """CRC32 of the little-endian int64 table: what the ranks of a data-parallel run compare before the first batch."""
    return zlib.crc32(np.ascontiguousarray(np.asarray(k, dtype="<i8")).tobytes()) & 0xFFFFFFFF
