"""Float64 CPU restatement of the SELD evaluation contract -- TEST infrastructure only; the product
(seld_eval.py, csrc/seld_eval.hip) never imports it.  Matching is by brute-force enumeration of the injections."""
from functools import lru_cache
from itertools import permutations

import numpy as np

WIN, HOP, FPM = 250, 50, 5
I, J, M, C = 18, 36, 14, 13
NEAR = 4e-5                # near-tie margin of the decode comparison


def cell_centre(cell, i_dim=I, j_dim=J):
    cell = np.asarray(cell, dtype=np.int64)
    return -180.0 + (cell % j_dim + 0.5) * (360.0 / j_dim), -90.0 + (cell // j_dim + 0.5) * (180.0 / i_dim)


def angle_deg(az1, el1, az2, el2):
    """Great-circle angle in degrees from the unit vectors (atan2 of |u x v| and u . v); identical directions are 0."""
    az1, el1, az2, el2 = (np.asarray(v, dtype=np.float64) for v in (az1, el1, az2, el2))
    rad = np.pi / 180.0
    a1, e1, a2, e2 = az1 * rad, el1 * rad, az2 * rad, el2 * rad
    u = np.stack([np.cos(e1) * np.cos(a1), np.cos(e1) * np.sin(a1), np.sin(e1)], -1)
    v = np.stack([np.cos(e2) * np.cos(a2), np.cos(e2) * np.sin(a2), np.sin(e2)], -1)
    cr = np.cross(u, v)
    d = np.arctan2(np.sqrt((cr ** 2).sum(-1)), (u * v).sum(-1)) * (180.0 / np.pi)
    return np.where((az1 == az2) & (el1 == el2), 0.0, d)


# ---------------------------------------------------------------------------------------------- meta-frames / decode

def meta_frames(segments):
    """[(first_frame, n_frames, segment, m)] in timeline order, by the label rule."""
    out = []
    for s, (first, n) in enumerate(np.asarray(segments, dtype=np.int64).reshape(-1, 2)):
        for m in range((int(n) + FPM - 1) // FPM):
            out.append((int(first) + FPM * m, min(FPM, int(n) - FPM * m), s, m))
    return out


def covering_windows(f, n_windows):
    lo = 0 if f < WIN else (f - WIN) // HOP + 1
    return range(lo, min(f // HOP, n_windows - 1) + 1)


def softmax64(x):
    x = np.asarray(x, dtype=np.float64)
    e = np.exp(x - x.max(-1, keepdims=True))
    return e / e.sum(-1, keepdims=True)


def decode_probs(window_logits, segments, total):
    """P_q [Q, 648, 13] in float64 from logits [W, 250, 648, 14] (any float dtype, used as given)."""
    n_w = (total + HOP - 1) // HOP
    assert window_logits.shape[0] == n_w
    mf = meta_frames(segments)
    out = np.zeros((len(mf), I * J, C))
    for q, (first, length, _, _) in enumerate(mf):
        acc = np.zeros((I * J, C))
        for f in range(first, first + length):
            ws = covering_windows(f, n_w)
            rows = np.stack([window_logits[w, f - HOP * w] for w in ws])
            acc += softmax64(rows)[..., :C].mean(0)
        out[q] = acc / length
    return out


def neighbours(cell):
    i, j = divmod(int(cell), J)
    for di in (-1, 0, 1):
        for dj in (-1, 0, 1):
            if (di or dj) and 0 <= i + di < I:
                yield (i + di) * J + (j + dj) % J


def decode_detections(probs, threshold, k):
    """probs P_q [Q, 648, 13] -> (dets: list over q of list over c of the peak cells sorted by (score desc, cell asc),
    first k; near: bool [Q, 13], the entries with a near tie: a candidate (P >= threshold - NEAR) within NEAR of the
    threshold or of a neighbour, or the k-th and (k+1)-th peaks within NEAR)."""
    q_n = probs.shape[0]
    g = probs.reshape(q_n, I, J, C)
    cell = np.arange(I * J).reshape(I, J)
    beats = np.ones(g.shape, bool)
    close = np.zeros(g.shape, bool)
    for di in (-1, 0, 1):
        for dj in (-1, 0, 1):
            if not (di or dj):
                continue
            ny = np.roll(g, -dj, axis=2)                     # ny[:, i, j] = g[:, i, (j + dj) mod J]
            yc = np.roll(cell, -dj, axis=1)
            valid = np.ones((I, J), bool)
            if di:
                ny = np.roll(ny, -di, axis=1)
                yc = np.roll(yc, -di, axis=0)
                valid[(I - 1) if di == 1 else 0, :] = False   # no wrap over the poles
            vb = valid[None, :, :, None]
            b = (g > ny) | ((g == ny) & (cell < yc)[None, :, :, None])
            beats &= b | ~vb
            close |= vb & (np.abs(g - ny) < NEAR)
    cand = g >= threshold - NEAR
    near = (cand & (close | (np.abs(g - threshold) < NEAR))).any(axis=(1, 2))
    peak = (beats & (g >= threshold)).reshape(q_n, I * J, C)
    flat = g.reshape(q_n, I * J, C)
    dets = []
    for q in range(q_n):
        row = []
        for c in range(C):
            xs = np.nonzero(peak[q, :, c])[0]
            order = sorted(xs.tolist(), key=lambda x: (-flat[q, x, c], x))
            if len(order) > k and abs(flat[q, order[k - 1], c] - flat[q, order[k], c]) < NEAR:
                near[q, c] = True
            row.append(order[:k])
        dets.append(row)
    return dets, near


def planted_logits(segments, seed):
    """Planted-peak window logits [W, 250, 648, 14] float32 for the decode test: N(0, 1) on every class with +4 on the
    background; per meta-frame 0-3 events at random (class, cell), every 4th meta-frame also 3-6 sources of one class;
    an event adds +8 at its cell for its frames and 4 + N(0, 0.5) on its neighbours; every window adds its own
    N(0, 0.3).  Rows past the timeline's end are N(0, 1)."""
    rng = np.random.default_rng(seed)
    segs = np.asarray(segments, dtype=np.int64).reshape(-1, 2)
    total = int((segs[:, 0] + segs[:, 1]).max())
    base = rng.standard_normal((total, I * J, M), dtype=np.float32)
    base[..., M - 1] += 4.0
    for q, (first, length, _, _) in enumerate(meta_frames(segs)):
        events = [(int(rng.integers(0, C)), int(rng.integers(0, I * J))) for _ in range(int(rng.integers(0, 4)))]
        if q % 4 == 0:
            c = int(rng.integers(0, C))
            events += [(c, int(rng.integers(0, I * J))) for _ in range(int(rng.integers(3, 7)))]
        for c, x in events:
            base[first:first + length, x, c] += 8.0
            for y in neighbours(x):
                base[first:first + length, y, c] += (4.0 + rng.normal(0.0, 0.5, size=length)).astype(np.float32)
    n_w = (total + HOP - 1) // HOP
    out = np.empty((n_w, WIN, I * J, M), dtype=np.float32)
    for w in range(n_w):
        n = min(WIN, total - HOP * w)
        out[w, :n] = base[HOP * w:HOP * w + n] + rng.normal(0.0, 0.3, size=(n, I * J, M)).astype(np.float32)
        out[w, n:] = rng.standard_normal((WIN - n, I * J, M), dtype=np.float32)
    return out


# ---------------------------------------------------------------------------------------------- matching / metrics

@lru_cache(maxsize=None)
def _injections(n, k):
    return np.array(list(permutations(range(n), k)), dtype=np.int64).reshape(-1, k)


def match_dist(dist, thr=20.0):
    """dist [R, P] (degrees) -> (k, tp, cost): brute force over every injection of the smaller side into the larger."""
    dist = np.asarray(dist, dtype=np.float64).reshape(len(dist), -1) if len(dist) else np.zeros((0, 0))
    r, p = dist.shape
    k = min(r, p)
    if k == 0:
        return 0, 0, 0.0
    d = dist if r <= p else dist.T
    inj = _injections(max(r, p), k)
    vals = d[np.arange(k)[None, :], inj]                       # [n_inj, k]
    return k, int((vals <= thr + 1e-6).sum(1).max()), float(vals.sum(1).min())


def match(ref_dirs, det_cells, thr=20.0):
    """References (az, el) [R, 2] vs detection cells [P] -> (R, P, k, tp, cost)."""
    ref_dirs = np.asarray(ref_dirs, dtype=np.float64).reshape(-1, 2)
    det_cells = np.asarray(det_cells, dtype=np.int64).reshape(-1)
    daz, del_ = cell_centre(det_cells)
    dist = angle_deg(ref_dirs[:, None, 0], ref_dirs[:, None, 1], daz[None, :], del_[None, :]) \
        if len(ref_dirs) and len(det_cells) else np.zeros((len(ref_dirs), len(det_cells)))
    k, tp, cost = match_dist(dist, thr)
    return len(ref_dirs), len(det_cells), k, tp, cost


def metrics(stats, cost):
    """stats [Q, 13, 4] = (R, P, k, tp), cost [Q, 13] -> the micro-averaged metrics, plain Python."""
    stats = np.asarray(stats, dtype=np.int64)
    cost = np.asarray(cost, dtype=np.float64)
    r, p, k, tp = (stats[..., i] for i in range(4))
    TP, FP, FN, N = int(tp.sum()), int((p - tp).sum()), int((r - tp).sum()), int(r.sum())
    S = D = Ins = 0
    for q in range(stats.shape[0]):
        fn, fp = int((r[q] - tp[q]).sum()), int((p[q] - tp[q]).sum())
        S += min(fn, fp)
        D += max(0, fn - fp)
        Ins += max(0, fp - fn)
    nan = float("nan")
    return {"TP": TP, "FP": FP, "FN": FN, "N": N, "S": S, "D": D, "I": Ins,
            "F20": 2 * TP / (2 * TP + FP + FN) if (2 * TP + FP + FN) else nan,
            "ER20": (S + D + Ins) / N if N else nan,
            "LE_CD": float(cost.sum()) / int(k.sum()) if k.sum() else nan,
            "LR_CD": int(k.sum()) / N if N else nan}
