"""numpy / float64 restatement of the rotation augmentation in azimuth steps, independent of
seld_augment.py and of csrc/rotate.hip: the test input (the "plane-wave clip"), the transformed recording and metadata, the
cell permutation, the rotation terms and the two identities the rotating gather rests on, and what the gather writes.

A window's transform: mirror m (az -> -az, Y -> -Y), then s cells of azimuth (az -> az + 360 s / J), then elevation flip e
(el -> -el, Z -> -Z).  With c = cos phi, sn = sin phi, phi = 2 pi s / J and sigma = -1 after a mirror, else +1:
    X' = c X - sn sigma Y        mel |X'|^2 = c^2 P_X + sn^2 P_Y - 2 c sn sigma C        IV_x' = c IV_x - sn sigma IV_y
    Y' = sn X + c sigma Y        mel |Y'|^2 = sn^2 P_X + c^2 P_Y + 2 c sn sigma C        IV_y' = sn IV_x + c sigma IV_y
with P_X = mel |X|^2, P_Y = mel |Y|^2, C = mel Re(X conj Y)."""
import math

import numpy as np
import torch

from oracle import features as ofeat

L = 24000                                   # samples of one clip: 51 feature frames, 50 label frames
I, J = 18, 36
SOURCES = ((35, 20, 3), (-110, -15, 7))     # (azimuth, elevation, class) of the two plane waves
STEP = 9                                    # parameter-row slot of the azimuth step


def plane_wave_clip(order="WYZX", index=0):
    """float32 [4, L] in ``order``: two independent N(0, 0.1^2) sources (torch seeds 1 and 2; clip ``index`` adds 3 * index
    to every seed) encoded as first-order plane waves at SOURCES -- W = s, X = s cos az cos el, Y = s sin az cos el,
    Z = s sin el -- plus independent noise at 0.1 x that level per channel (seed 3)."""
    def normal(seed, *shape):
        return torch.randn(*shape, generator=torch.Generator().manual_seed(seed + 3 * index), dtype=torch.float64).numpy()
    field = {k: np.zeros(L) for k in "WXYZ"}
    for n, (az, el, _) in enumerate(SOURCES):
        s = 0.1 * normal(1 + n, L)
        a, b = math.radians(az), math.radians(el)
        field["W"] += s
        field["X"] += s * math.cos(a) * math.cos(b)
        field["Y"] += s * math.sin(a) * math.cos(b)
        field["Z"] += s * math.sin(b)
    noise = 0.01 * normal(3, 4, L)
    return torch.from_numpy(np.stack([field[k] + noise[n] for n, k in enumerate(order)]).astype(np.float32))


def clip_rows():
    """Metadata of one plane-wave clip: both sources active in all ten 100 ms frames, int64 [20, 5].  The DOAs are the
    encoding angles moved one degree off the cell edges (20 -> 21, -110 -> -109): polar_to_grid truncates, so a direction ON
    an edge does not commute with the mirror or the flip (tests/test_augment_cpu.py), and the label transform is defined on
    cells for that reason.  Labels never look at the audio, nor features at the metadata."""
    def off_edge(v, top):
        return v if v % 10 else (v - 1 if v >= top else v + 1)
    return np.asarray([(t, cls, n, off_edge(az, 175), off_edge(el, 85)) for t in range(10)
                       for n, (az, el, cls) in enumerate(SOURCES)], dtype=np.int64)


def angle(s, steps=J):
    return 2.0 * math.pi * (s % steps) / steps


def doa(m, s, e, az, el, steps=J):
    """One DOA (integer degrees) through (m, s, e); az' wrapped to [-180, 180)."""
    az = -az if m else az
    az = (az + (360 // steps) * s + 180) % 360 - 180
    return az, (-el if e else el)


def rows_transformed(rows, m, s, e, steps=J):
    out = np.array(rows, dtype=np.int64, copy=True)
    for r in out:
        r[3], r[4] = doa(m, s, e, int(r[3]), int(r[4]), steps)
    return out


def field_transformed(x, y, z, m, s, e, steps=J):
    """(X, Y, Z) of a sound field -> those of the transformed field, float64."""
    c, sn = math.cos(angle(s, steps)), math.sin(angle(s, steps))
    sigma = -1.0 if m else 1.0
    return c * x - sn * sigma * y, sn * x + c * sigma * y, (-z if e else z)


def pcm_transformed(pcm, m, s, e, order="WYZX", steps=J):
    """float64 [4, L] clip of the transformed sound field, channels in ``order``."""
    pcm = np.asarray(pcm, dtype=np.float64)
    ch = {letter: pcm[n] for n, letter in enumerate(order)}
    x, y, z = field_transformed(ch["X"], ch["Y"], ch["Z"], m, s, e, steps)
    new = {"W": ch["W"], "X": x, "Y": y, "Z": z}
    return np.stack([new[letter] for letter in order])


def permute_cells(mask, m, s, e, I=I, J=J):
    """mask [..., I*J] -> the same with every cell (i, j) moved to (e ? I-1-i : i, ((m ? J-1-j : j) + s) mod J)."""
    out = np.zeros_like(mask)
    for i in range(I):
        for j in range(J):
            i2 = I - 1 - i if e else i
            j2 = ((J - 1 - j if m else j) + s) % J
            out[..., i2 * J + j2] = mask[..., i * J + j]
    return out


def rotation_terms_f64(pcm, order="WYZX"):
    """float64 [3, 64, F]: P_X, P_Y, C of a 4-channel clip."""
    spec = ofeat.stft_f64(np.asarray(pcm, dtype=np.float64))                       # [4, 481, F]
    x, y = spec[order.index("X")], spec[order.index("Y")]
    fb = ofeat.mel_filterbank_htk().numpy().astype(np.float64)
    products = np.stack([np.abs(x) ** 2, np.abs(y) ** 2, (x * np.conj(y)).real])
    return np.einsum("cft,fm->cmt", products, fb)


def combined_powers(px, py, cross, c, sn, m):
    """(mel |X'|^2, mel |Y'|^2) from the three terms; float64 arrays or scalars, (c, sn) as given."""
    px, py, cross = (np.asarray(v, dtype=np.float64) for v in (px, py, cross))
    c, sn = float(c), float(sn)
    g = 2.0 * c * sn * (-1.0 if m else 1.0) * cross
    return c * c * px + sn * sn * py - g, sn * sn * px + c * c * py + g


def cancellation(px, py, cross_magnitude, c, sn, vx, vy):
    """(kappa of X', kappa of Y'): the sum of the magnitudes of the three terms over the rotated power v."""
    px, py, cm = (np.asarray(v, dtype=np.float64) for v in (px, py, cross_magnitude))
    c, sn = float(c), float(sn)
    g = 2.0 * abs(c * sn) * cm
    with np.errstate(divide="ignore", invalid="ignore"):
        return (c * c * px + sn * sn * py + g) / vx, (sn * sn * px + c * c * py + g) / vy


def split(p):
    return (p >> 3) & 1, (p >> 1) & 3, p & 1


def gather(spec_tm, rot_tm, mask_tm, starts, params, window, table, order="WYZX", channel_table=None, freq_channels=None,
           mask_value=0.0, I=I, J=J):
    """What the rotating pair writes for ROTATED windows and what bounds it, from the device's own fp32 timeline:
    returns (want float64 [B, window, C, 64], tol float64 same shape, computed bool same shape (False: a copied, masked or
    zero element, bit-equal to ``want`` cast to fp32), floor_ok bool same shape (the -100 dB floor is also accepted),
    labels uint16 [B, window, I*J], rotated bool [B]).
    ``table`` float32 [J, 2] (cos, sin).  Windows whose total step is a whole number of quarter turns are left to the
    bit-equality tests: their rows of ``want`` hold the signed channel copy of ``channel_table``."""
    spec_tm = np.ascontiguousarray(spec_tm, dtype=np.float32)
    rot = np.asarray(rot_tm, dtype=np.float64)
    total, C, bins = spec_tm.shape
    freq_channels = C if freq_channels is None else freq_channels
    cx, cy, cz = order.index("X"), order.index("Y"), order.index("Z")
    B = len(starts)
    want = np.zeros((B, window, C, bins))
    tol = np.zeros_like(want)
    computed = np.zeros(want.shape, dtype=bool)
    floor_ok = np.zeros(want.shape, dtype=bool)
    labels = np.zeros((B, window, I * J), dtype=np.uint16)
    rotated = np.zeros(B, dtype=bool)
    fill = float(np.float32(mask_value))
    for b in range(B):
        row = [int(v) for v in params[b]]
        m, k, e = split(row[0] & 15)
        s = (k * (J // 4) + row[STEP] % J) % J
        first = int(starts[b])
        n = max(0, min(window, total - first))
        if n == 0:
            continue
        src = spec_tm[first:first + n].astype(np.float64)
        out = want[b, :n]
        if s % (J // 4) == 0:
            p = (m << 3) | ((s // (J // 4)) << 1) | e
            for c in range(C):
                entry = int(channel_table[p][c])
                out[:, c] = -src[:, entry & 0x7f] if entry & 0x80 else src[:, entry & 0x7f]
        else:
            rotated[b] = True
            c_, sn = float(table[s][0]), float(table[s][1])
            sigma = -1.0 if m else 1.0
            out[:, 0], out[:, cz] = src[:, 0], src[:, cz]
            px, py, cross = rot[first:first + n, 0], rot[first:first + n, 1], rot[first:first + n, 2]
            vx, vy = combined_powers(px, py, cross, c_, sn, m)
            kx, ky = cancellation(px, py, np.abs(cross), c_, sn, vx, vy)
            for c, v, kappa in ((cx, vx, kx), (cy, vy, ky)):
                out[:, c] = 10.0 * np.log10(np.maximum(v, 1e-10))
                out[:, c][v <= 1e-10] = -100.0
                tol[b, :n, c] = 1e-5 + 1.1e-6 * np.where(np.isfinite(kappa) & (kappa > 0), kappa, 0.0)
                floor_ok[b, :n, c] = v < 2e-10
                computed[b, :n, c] = True
            if C == 7:
                out[:, 3 + cz] = -src[:, 3 + cz] if e else src[:, 3 + cz]
                ix, iy = src[:, 3 + cx], src[:, 3 + cy]
                out[:, 3 + cx] = c_ * ix - sn * sigma * iy
                out[:, 3 + cy] = sn * ix + c_ * sigma * iy
                tol[b, :n, 3 + cx] = 3 * 2.0 ** -24 * (np.abs(c_ * ix) + np.abs(sn * iy))
                tol[b, :n, 3 + cy] = 3 * 2.0 ** -24 * (np.abs(sn * ix) + np.abs(c_ * iy))
                computed[b, :n, 3 + cx] = computed[b, :n, 3 + cy] = True
        for t0, tl in ((row[1], row[2]), (row[3], row[4])):
            stop = min(t0 + tl, n)
            want[b, t0:stop], tol[b, t0:stop], floor_ok[b, t0:stop], computed[b, t0:stop] = fill, 0.0, False, False
        for f0, fl in ((row[5], row[6]), (row[7], row[8])):
            want[b, :n, :freq_channels, f0:f0 + fl] = fill
            tol[b, :n, :freq_channels, f0:f0 + fl] = 0.0
            floor_ok[b, :n, :freq_channels, f0:f0 + fl] = False
            computed[b, :n, :freq_channels, f0:f0 + fl] = False
        labels[b, :n] = permute_cells(mask_tm[first:first + n], m, s, e, I, J)
    return want, tol, computed, floor_ok, labels, rotated
