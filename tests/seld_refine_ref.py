"""Float64 CPU restatement of the sub-cell DOA refinement and the synthetic maps its tests share
-- TEST infrastructure only; the product (seld_eval.py, csrc/seld_refine.hip) never imports it."""
from functools import lru_cache

import numpy as np

import seld_eval_ref as ref

I, J, C = ref.I, ref.J, ref.C
SIGMA_DEG = 6.0            # angular width of the synthetic bumps
AMPLITUDE = 0.3
BUMP_THRESHOLD = 0.1       # a source at a cell corner keeps 0.50 of its amplitude at the peak: 0.15 >= 0.1


def unit(az_deg, el_deg):
    """(cos el cos az, cos el sin az, sin el) in float64, [..., 3]."""
    az, el = np.deg2rad(np.asarray(az_deg, dtype=np.float64)), np.deg2rad(np.asarray(el_deg, dtype=np.float64))
    return np.stack([np.cos(el) * np.cos(az), np.cos(el) * np.sin(az), np.sin(el)], axis=-1)


@lru_cache(maxsize=None)
def cell_units(fp32=True):
    """u(y) of every cell centre [648, 3]: float64, rounded to fp32 (the table the kernel is handed) when ``fp32``."""
    u = unit(*ref.cell_centre(np.arange(I * J)))
    u = u.astype(np.float32).astype(np.float64) if fp32 else u
    u.setflags(write=False)
    return u


def neighbourhood(cell):
    """N(x) in the summation order: di = -1, 0, 1 outer, dj = -1, 0, 1 inner, the centre included; azimuth wraps, no wrap
    over the poles."""
    i, j = divmod(int(cell), J)
    return [(i + di) * J + (j + dj) % J for di in (-1, 0, 1) if 0 <= i + di < I for dj in (-1, 0, 1)]


def refine(class_map, cell, fp32_sum=False):
    """(az, el) in degrees of the detection at ``cell`` of one class map P[648] (used as given).  Float64 throughout, or
    with ``fp32_sum`` the products and the running sums rounded to fp32 (the kernel's precision, unfused)."""
    u = cell_units()
    p = np.asarray(class_map)
    if fp32_sum:
        v = np.zeros(3, np.float32)
        for y in neighbourhood(cell):
            v = (v + np.float32(p[y]) * u[y].astype(np.float32)).astype(np.float32)
        v = v.astype(np.float64)
    else:
        v = np.zeros(3)
        for y in neighbourhood(cell):
            v = v + float(p[y]) * u[y]
    n2 = float((v * v).sum())
    if not (n2 > 0.0 and np.isfinite(n2)):
        az, el = ref.cell_centre(cell)
        return float(az), float(el)
    az = float(np.degrees(np.arctan2(v[1], v[0])))
    el = float(np.degrees(np.arctan2(v[2], np.hypot(v[0], v[1]))))
    return (-180.0 if az >= 180.0 else az), el


def refine_detections(probs, det_cell, det_count):
    """probs P_q [Q, 648, 13], the kernel's cells [Q, 13, K] and counts [Q, 13] -> float64 [Q, 13, K, 2], 0 past the
    count."""
    det_cell, det_count = np.asarray(det_cell), np.asarray(det_count)
    out = np.zeros(det_cell.shape + (2,))
    for q, c in zip(*np.nonzero(det_count)):
        for r in range(int(det_count[q, c])):
            out[q, c, r] = refine(probs[q, :, c], det_cell[q, c, r])
    return out


def angle(a, b):
    """Great-circle angle in degrees between directions a and b, [..., 2] = (az, el)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return ref.angle_deg(a[..., 0], a[..., 1], b[..., 0], b[..., 1])


@lru_cache(maxsize=None)
def bump_maps(seed, n_meta=100, n_sources=3, sigma_deg=SIGMA_DEG, hold=1):
    """Synthetic class maps of one segment of ``n_meta`` meta-frames: per meta-frame ``n_sources`` sources of distinct
    classes with true directions uniform on the sphere, |el| <= 80; P[y][c] = 0.3 exp((u(y) . s - 1) / sigma^2), the
    background 1 - sum; the sources are drawn anew every ``hold`` meta-frames and hold still between.  Returns (P float64
    [n_meta, 648, 14], sources [(q, c, az, el)]).  Shared: do not write."""
    rng = np.random.default_rng(seed)
    u = cell_units(fp32=False)
    s2 = np.deg2rad(sigma_deg) ** 2
    probs = np.zeros((n_meta, I * J, C + 1))
    sources = []
    for q in range(n_meta):
        if q % hold == 0:
            lim = np.sin(np.deg2rad(80.0))
            drawn = [(int(c), float(rng.uniform(-180.0, 180.0)), float(np.degrees(np.arcsin(rng.uniform(-lim, lim)))))
                     for c in rng.choice(C, size=n_sources, replace=False)]
        for c, az, el in drawn:
            probs[q, :, c] = AMPLITUDE * np.exp((u @ unit(az, el) - 1.0) / s2)
            sources.append((q, c, az, el))
    probs[..., C] = 1.0 - probs[..., :C].sum(-1)
    assert probs[..., C].min() > 0.0
    probs.setflags(write=False)
    return probs, tuple(sources)


def bump_errors(probs, sources):
    """Decode the maps with the restatement (threshold 0.1, K = 8) -> (detections, centre errors, refined errors): every
    source's detection of its class, its cell centre's and its refined direction's angle to the true direction."""
    dets, _ = ref.decode_detections(probs[..., :C], BUMP_THRESHOLD, 8)
    n_det = sum(len(row) for per_q in dets for row in per_q)
    centre, refined = [], []
    for q, c, az, el in sources:
        if len(dets[q][c]) != 1:
            continue
        x = dets[q][c][0]
        centre.append(float(angle(np.array(ref.cell_centre(x), dtype=np.float64), (az, el))))
        refined.append(float(angle(refine(probs[q, :, c], x), (az, el))))
    return n_det, np.array(centre), np.array(refined)
