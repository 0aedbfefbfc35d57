"""Plain restatements of class-balanced window sampling for the tests: the two kernels of
csrc/balance.hip in numpy, and the weights, their quantisation and the epoch's order of seld_balance.py in Python loops over
Python floats and ints -- nothing here imports the code under test."""
import bisect
import math

import numpy as np

COLUMNS = 16
MAX_CLASSES = 14


def frame_class_mask(mask):
    """uint16 [T]: the bitwise OR over the cells of every row of mask uint16 [T, cells]."""
    mask = np.asarray(mask, dtype=np.uint16)
    return np.bitwise_or.reduce(mask, axis=1).astype(np.uint16)


def window_class_frames(frame_mask, window, hop, n_windows, num_classes):
    """int32 [n_windows, 16] from the per-frame words: class columns, frames with any class (14), frames in the timeline (15);
    bits at or above num_classes are ignored."""
    frame_mask = np.asarray(frame_mask, dtype=np.uint16)
    total = len(frame_mask)
    counts = np.zeros((n_windows, COLUMNS), dtype=np.int32)
    keep = np.uint16((1 << num_classes) - 1)
    for w in range(n_windows):
        rows = frame_mask[w * hop:min(w * hop + window, total)] & keep
        for c in range(num_classes):
            counts[w, c] = int(((rows >> np.uint16(c)) & np.uint16(1)).sum())
        counts[w, 14] = int((rows != 0).sum())
        counts[w, 15] = len(rows)
    return counts


def window_weights(counts, power, silent_share, min_frames):
    """The int64 table k, one window at a time."""
    counts = np.asarray(counts)
    n = len(counts)
    present = [[int(counts[w][c]) >= min_frames for c in range(MAX_CLASSES)] for w in range(n)]
    holders = [sum(1 for w in range(n) if present[w][c]) for c in range(MAX_CLASSES)]
    weight = [0.0] * n
    active, silent = [], []
    for w in range(n):
        mine = [math.pow(float(holders[c]), -power) for c in range(MAX_CLASSES) if present[w][c]]
        if mine:
            weight[w] = max(mine)
            active.append(w)
        else:
            silent.append(w)
    if not active:
        raise ValueError("no active window")
    if silent:
        share = len(silent) / n if silent_share is None else silent_share
        each = (share * math.fsum(weight[w] for w in active)) / ((1.0 - share) * len(silent))
        for w in silent:
            weight[w] = each
    top = max(weight)
    k = []
    for w in range(n):
        q = int(math.floor(weight[w] / top * 4294967296.0 + 0.5))
        k.append(max(q, 1) if weight[w] > 0 else 0)
    return np.array(k, dtype=np.int64)


def order(k, seed, epoch):
    """The epoch's window indices: every draw looked up in the running sum of k."""
    k = [int(v) for v in k]
    total = sum(k)
    u = np.random.default_rng([seed, epoch, 0, 3]).integers(0, total, size=len(k), dtype=np.int64)
    cum, run = [], 0
    for v in k:
        run += v
        cum.append(run)
    # the first window whose running sum exceeds the draw
    return np.array([bisect.bisect_right(cum, draw) for draw in u.tolist()], dtype=np.int64)
