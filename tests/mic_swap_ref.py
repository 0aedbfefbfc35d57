"""numpy restatement of the channel swap of microphone-array features, independent of
seld_augment.py and of csrc/micswap.hip: the microphone permutation of a pattern from the positions, the operation per
feature channel, the affine map, the masks and the zero rows -- in float32 where the kernel is float32.

Pattern p acts on a direction (x, y, z): mirror m = p >> 3 (y -> -y), then k = (p >> 1) & 3 quarter turns ((x, y) -> (-y, x)),
then flip e = p & 1 (z -> -z): T_p.  p is valid for positions r_0..r_{C-1} when {T_p^-1 r_j} is the same point set;
sigma_p(j) is then the index with r[sigma_p(j)] = T_p^-1 r[j], and the transformed scene's channel j is the recording's
channel sigma_p(j)."""
import numpy as np

from augment_ref import permute_cells

TETRA_ANGLES = ((45, 35), (-45, -35), (135, -35), (-135, 35))       # (azimuth, elevation) in degrees, 4.2 cm
TETRA_SIGMA = {0: [0, 1, 2, 3], 3: [1, 3, 0, 2], 4: [3, 2, 1, 0], 7: [2, 0, 3, 1], 9: [1, 0, 3, 2], 10: [0, 2, 1, 3],
               13: [2, 3, 0, 1], 14: [3, 1, 2, 0]}


def unit(az_deg, el_deg):
    az, el = np.radians(az_deg), np.radians(el_deg)
    return np.array([np.cos(az) * np.cos(el), np.sin(az) * np.cos(el), np.sin(el)])


def tetrahedron():
    return 0.042 * np.stack([unit(az, el) for az, el in TETRA_ANGLES])


def cube(half=0.05):
    return half * np.array([(x, y, z) for x in (-1.0, 1.0) for y in (-1.0, 1.0) for z in (-1.0, 1.0)])


def apply_pattern(p, v):
    """T_p on vectors [..., 3]."""
    x, y, z = v[..., 0], v[..., 1], v[..., 2]
    if p >> 3:
        y = -y
    for _ in range((p >> 1) & 3):
        x, y = -y, x
    if p & 1:
        z = -z
    return np.stack([x, y, z], axis=-1)


def apply_inverse(p, v):
    """T_p^-1: the three steps undone in reverse order."""
    x, y, z = v[..., 0], v[..., 1], v[..., 2]
    if p & 1:
        z = -z
    for _ in range((p >> 1) & 3):
        x, y = y, -x
    if p >> 3:
        y = -y
    return np.stack([x, y, z], axis=-1)


def sigma(positions, p):
    """The permutation of pattern p as a list, or None when p is no symmetry of the array."""
    pos = np.asarray(positions, dtype=np.float64)
    tol = 1e-3 * np.linalg.norm(pos, axis=1).max()
    moved = apply_inverse(p, pos)
    out, used = [], set()
    for j in range(len(pos)):
        hits = [i for i in range(len(pos)) if np.linalg.norm(pos[i] - moved[j]) <= tol]
        if len(hits) != 1 or hits[0] in used:
            return None
        used.add(hits[0])
        out.append(hits[0])
    return out


def valid_patterns(positions):
    return [p for p in range(16) if sigma(positions, p) is not None]


def pair_index(a, b, C):
    """Place of the pair (a, b), a < b, among the lexicographic pairs of C microphones."""
    pairs = [(i, j) for i in range(C) for j in range(i + 1, C)]
    return pairs.index((a, b))


def transform_rows(rows, sig, kind):
    """rows float32 [n, channels, 64] of stored features -> the features of the scene whose channel j is the recording's
    channel sig[j].  kind 'gcc': C + C(C-1)/2 channels; 'nipd': 2C - 1; 'logmel': C.  float64 rows stay float64 (the
    rule itself, for the CPU tests); anything else is taken as the kernel's float32."""
    rows = np.asarray(rows)
    if rows.dtype != np.float64:
        rows = rows.astype(np.float32)
    C = len(sig)
    out = np.empty_like(rows)
    for c in range(C):
        out[:, c] = rows[:, sig[c]]
    if kind == "logmel":
        assert rows.shape[1] == C
    elif kind == "gcc":
        assert rows.shape[1] == C + C * (C - 1) // 2
        for a in range(C):
            for b in range(a + 1, C):
                u, v = sig[a], sig[b]
                dst = C + pair_index(a, b, C)
                if u < v:
                    out[:, dst] = rows[:, C + pair_index(u, v, C)]
                else:
                    stored = rows[:, C + pair_index(v, u, C)]
                    out[:, dst, 0] = stored[:, 0]                   # lag +32 is not stored: the -32 slot stays
                    out[:, dst, 1:] = stored[:, :0:-1]              # out[j] = in[64 - j], j = 1..63
    else:
        assert kind == "nipd" and rows.shape[1] == 2 * C - 1
        zero = np.zeros(rows.shape[:1] + rows.shape[2:], dtype=rows.dtype)      # N(0) = +0.0
        N = lambda i: zero if i == 0 else rows[:, C + i - 1]
        for m in range(1, C):
            if sig[0] == 0:
                out[:, C + m - 1] = N(sig[m])
            else:
                out[:, C + m - 1] = (N(sig[m]) - N(sig[0])).astype(rows.dtype)      # one subtraction in the rows' format
    return out


def fma32(v, scale, shift):
    """float32 fma(v, scale, shift) of float32 operands, exactly: the float64 product of two float32 values is exact, the
    float64 sum s of it and the shift rounds once, and TwoSum gives what that rounding lost.  s rounded to float32 is the
    fused result unless s lies exactly half way between two float32 values while the true sum does not -- a float32
    midpoint is a float64 number, so the true sum and s can never lie on different sides of one -- and there the lost part's
    sign decides."""
    v, scale, shift = (np.asarray(a, dtype=np.float32).astype(np.float64) for a in (v, scale, shift))
    p = v * scale
    s = p + shift
    t = s - p
    lost = (p - (s - t)) + (shift - t)                              # TwoSum: p + shift == s + lost, exactly
    r = s.astype(np.float32)
    away = np.where(r.astype(np.float64) > s, np.float32(-np.inf), np.float32(np.inf))
    other = np.nextafter(r, away)                                   # the float32 neighbour on the far side of s
    tie = (r.astype(np.float64) != s) & ((r.astype(np.float64) + other.astype(np.float64)) / 2 == s) & (lost != 0)
    towards_other = tie & (np.sign(lost) == np.sign(other.astype(np.float64) - s))
    return np.where(towards_other, other, r).astype(np.float32)


def gather(spec_tm, mask_tm, starts, params, window, positions, kind, freq_channels=None, mask_value=0.0, scale=None,
           shift=None, I=18, J=36):
    """What the array gather and the label gather write: (spec float32 [B, window, channels, 64], mask uint16 [B, window,
    I*J]).  Per window: rows starts[b] + w inside the timeline are transformed by the pattern of params[b] (the identity
    when it is no symmetry of the array), then float32 fma(v, scale, shift) (``fma32``: exact for any tables), then the
    time masks (every channel) and the frequency masks (channels < freq_channels) set elements to mask_value; rows outside
    the timeline are +0.0 whatever the masks say; labels are permuted and never masked.  mask_tm None: no labels."""
    spec_tm = np.ascontiguousarray(spec_tm, dtype=np.float32)
    total, channels, bins = spec_tm.shape
    freq_channels = channels if freq_channels is None else freq_channels
    C = len(positions)
    B = len(starts)
    spec = np.zeros((B, window, channels, bins), dtype=np.float32)
    mask = None if mask_tm is None else np.zeros((B, window, I * J), dtype=np.uint16)
    fill = np.float32(mask_value)
    moved = {}                                                      # the whole timeline under a pattern, once
    for b in range(B):
        row = [int(v) for v in params[b]]
        p = row[0] & 15
        if p not in moved:
            v = transform_rows(spec_tm, sigma(positions, p) or list(range(C)), kind)
            if scale is not None:
                v = fma32(v, scale, shift)
            moved[p] = v
        s0 = int(starts[b])
        lo, hi = max(0, -s0), min(window, total - s0)               # frames [lo, hi) of the window lie on the timeline
        if hi <= lo:
            continue
        v = moved[p][s0 + lo:s0 + hi].copy()
        for f0, fl in ((row[5], row[6]), (row[7], row[8])):
            if fl > 0:
                v[:, :freq_channels, f0:f0 + fl] = fill
        spec[b, lo:hi] = v
        for t0, tl in ((row[1], row[2]), (row[3], row[4])):
            if tl > 0:
                spec[b, max(t0, lo):min(t0 + tl, hi)] = fill
        if mask is not None:
            mask[b, lo:hi] = permute_cells(mask_tm[s0 + lo:s0 + hi], p, I, J)
    return spec, mask
