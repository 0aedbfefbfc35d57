"""numpy restatement of the in-place spectral stage, independent of seld_augment.py and of
csrc/spectral.hip: what the stage writes, element by element, from a gathered batch, the windows' starts, their parameter
rows, their spectral rows and their gain curves.

Per window b, frame w, channel c, bin f, in this order:
  1. row starts[b] + w outside [0, total_rows): the row stays as it is;
  2. c < freq_channels: v = x[b, w, c, clamp(f - s, 0, 63)], else v = x[b, w, c, f];
  3. c < logmel_channels and flag bit 0 set: v <= -100 stays, else v = max(v + G[b, f], -100);
  4. with statistics: v = v * scale[c, f] + shift[c, f];
  5. the time / frequency masks of the parameter row, then the two cutouts (channels < freq_channels): mask_value.
"""
import numpy as np

BINS = 64
ROW_INTS = 12
FLOOR = -100.0


def in_span(x, start, length):
    """x in [start, start + length) for integer arrays / scalars of any size, without overflow."""
    x, start, length = np.asarray(x, dtype=object), int(start), int(length)
    return np.asarray((length > 0) & (x >= start) & (x - start < length), dtype=bool)


def rows(shifts, curves_on=None, cutouts=None):
    """int32 [B, 12] spectral rows from lists: shift per window, flag per window, ((t, tl, f0, fl), (t, tl, f0, fl)) per
    window."""
    out = np.zeros((len(shifts), ROW_INTS), dtype=np.int32)
    out[:, 0] = shifts
    if curves_on is not None:
        out[:, 1] = np.asarray(curves_on, dtype=np.int32)
    if cutouts is not None:
        for b, pair in enumerate(cutouts):
            out[b, 2:10] = np.asarray(pair, dtype=np.int64).reshape(8)
    return out


def stage(x, starts, total_rows, params, spectral, curves, logmel_channels, freq_channels, mask_value, scale=None, shift=None,
          dtype=np.float32):
    """The stage on x [B, W, C, 64].  ``dtype`` float32: every arithmetic step in fp32 (the addition one IEEE addition; the map
    as v * scale + shift, which is the fused multiply-add's rounding for power-of-two scales); float64: the same steps
    evaluated in double precision from the fp32 inputs.  ``params`` / ``curves`` None: no masks / no curve for any window."""
    x = np.asarray(x)
    B, W, C, bins = x.shape
    assert bins == BINS and 0 <= logmel_channels <= freq_channels <= C
    out = x.astype(dtype).copy()
    f = np.arange(BINS)
    frames = np.arange(W)
    mask_value = dtype(mask_value)
    for b in range(B):
        live = np.asarray([0 <= int(starts[b]) + int(w) < int(total_rows) for w in frames])
        s = max(-BINS, min(BINS, int(spectral[b][0])))
        v = x[b].astype(dtype).copy()                                               # [W, C, 64]
        v[:, :freq_channels] = x[b][:, :freq_channels][:, :, np.clip(f - s, 0, BINS - 1)].astype(dtype)
        if curves is not None and (int(spectral[b][1]) & 1) and logmel_channels:
            g = np.asarray(curves[b]).astype(dtype)                                 # float64 curves stay float64 there
            head = v[:, :logmel_channels]
            v[:, :logmel_channels] = np.where(head <= dtype(FLOOR), head, np.maximum(head + g, dtype(FLOOR)))
        if scale is not None:
            v = (v * np.asarray(scale, dtype=np.float32).astype(dtype) + np.asarray(shift, dtype=np.float32).astype(dtype)).astype(dtype)
        hit = np.zeros((W, C, BINS), dtype=bool)
        if params is not None:
            p = [int(n) for n in params[b]]
            hit |= (in_span(frames, p[1], p[2]) | in_span(frames, p[3], p[4]))[:, None, None]
            hit[:, :freq_channels] |= (in_span(f, p[5], p[6]) | in_span(f, p[7], p[8]))[None, None, :]
        for first in (2, 6):
            t, tl, f0, fl = (int(n) for n in spectral[b][first:first + 4])
            hit[:, :freq_channels] |= (in_span(frames, t, tl)[:, None] & in_span(f, f0, fl)[None, :])[:, None, :]
        v[hit] = mask_value
        out[b][live] = v[live]
    return out


def draw_row(seed, epoch, index, shift_max, level_db, cutouts, time_max, freq_max, filter_prob, filter_db, bands, kind, window):
    """The draw of DESIGN.md section 26.3 restated: one window's (row int32 [12], curve float32 [64] or None, number of
    bands or 0).  Every question in a fixed order from default_rng([seed, epoch, index, 2]), each one random()."""
    rng = np.random.default_rng([seed, epoch, index, 2])
    pick = lambda u, count: min(int(u * count), count - 1)
    row = np.zeros(ROW_INTS, dtype=np.int32)
    row[0] = pick(rng.random(), 2 * shift_max + 1) - shift_max
    level = (2.0 * rng.random() - 1.0) * level_db
    for n in range(2):
        u = rng.random(4)
        tl = pick(u[0], min(time_max, window) + 1)
        t = pick(u[1], window - tl + 1)
        fl = pick(u[2], min(freq_max, BINS) + 1)
        f0 = pick(u[3], BINS - fl + 1)
        if n < cutouts:
            row[2 + 4 * n:6 + 4 * n] = (t, tl, f0, fl)
    filtered = rng.random() < filter_prob
    if not filtered and level_db == 0:
        return row, None, 0
    curve = np.full(BINS, level, dtype=np.float64)
    n = 0
    if filtered:
        n = int(rng.integers(bands[0], bands[1] + 1))
        inner = np.sort(rng.choice(np.arange(1, BINS), size=n - 1, replace=False)) if n > 1 else np.zeros(0, dtype=np.int64)
        edges = np.concatenate([[0], inner, [BINS]])
        if kind == "step":
            gains = rng.uniform(-filter_db, filter_db, n)
            for k in range(n):
                curve[edges[k]:edges[k + 1]] += gains[k]
        else:
            gains = rng.uniform(-filter_db, filter_db, n + 1)
            for k in range(n):
                span = np.arange(edges[k], edges[k + 1])
                curve[span] += gains[k] + (gains[k + 1] - gains[k]) * (span - edges[k]) / float(edges[k + 1] - edges[k])
    row[1] = 1
    return row, curve.astype(np.float32), n
