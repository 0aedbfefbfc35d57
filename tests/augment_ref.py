"""numpy restatement of the training augmentation, independent of seld_augment.py and of the kernels:
the tests hold csrc/augment.hip and the host tables to THIS, and this to the oracle's rasteriser / feature code.

Pattern p in 0..15: mirror m = p >> 3 (az -> -az, Y -> -Y), then k = (p >> 1) & 3 quarter turns (az -> az + 90 k), then
elevation flip e = p & 1 (el -> -el, Z -> -Z)."""
import numpy as np

PARAM_INTS = 12


def split(p):
    return (p >> 3) & 1, (p >> 1) & 3, p & 1


def doa(p, az, el):
    """One DOA (integer degrees) through pattern p; az' wrapped to [-180, 180)."""
    m, k, e = split(p)
    az = -az if m else az
    az = (az + 90 * k + 180) % 360 - 180
    return az, (-el if e else el)


def rows_transformed(rows, p):
    """Metadata rows [R, 5] = (meta_frame, class, source, az, el) with every DOA moved by pattern p."""
    out = np.array(rows, dtype=np.int64, copy=True)
    for r in out:
        r[3], r[4] = doa(p, int(r[3]), int(r[4]))
    return out


def off_edge_rows(rows):
    """Nudge any DOA on a cell edge (az % 10 == 0 or el % 10 == 0) by one degree: polar_to_grid truncates, so only
    directions off the edges commute with a mirror; the label transform is defined on cells for that reason."""
    out = np.array(rows, dtype=np.int64, copy=True)
    out[:, 3] = np.where(out[:, 3] % 10 == 0, np.where(out[:, 3] >= 175, out[:, 3] - 1, out[:, 3] + 1), out[:, 3])
    out[:, 4] = np.where(out[:, 4] % 10 == 0, np.where(out[:, 4] >= 85, out[:, 4] - 1, out[:, 4] + 1), out[:, 4])
    return out


def permute_cells(mask, p, I=18, J=36):
    """mask [..., I*J] -> the same with every cell (i, j) moved to (e ? I-1-i : i, ((m ? J-1-j : j) + k J/4) mod J)."""
    m, k, e = split(p)
    out = np.zeros_like(mask)
    for i in range(I):
        for j in range(J):
            i2 = I - 1 - i if e else i
            j2 = ((J - 1 - j if m else j) + k * (J // 4)) % J
            out[..., i2 * J + j2] = mask[..., i * J + j]
    return out


def field_transformed(x, y, z, p):
    """(X, Y, Z) components of a sound field -> those of the transformed field (any array type with unary minus)."""
    m, k, e = split(p)
    if m:
        y = -y
    x, y = ((x, y), (-y, x), (-x, -y), (y, -x))[k]
    return x, y, (-z if e else z)


def pcm_transformed(pcm, p, order="WYZX"):
    """A 4-channel FOA clip [4, L] (channels in ``order``) -> the clip of the transformed sound field, same order."""
    ch = {letter: pcm[n] for n, letter in enumerate(order)}
    x, y, z = field_transformed(ch["X"], ch["Y"], ch["Z"], p)
    new = {"W": ch["W"], "X": x, "Y": y, "Z": z}
    return np.stack([np.asarray(new[letter]) for letter in order])


def gather(spec_tm, mask_tm, starts, params, window, channel_table=None, freq_channels=None, mask_value=0.0, I=18, J=36):
    """What the two augmenting gathers write: (spec float32 [B, window, C, 64], mask uint16 [B, window, I*J]).
    spec[b, w, c, f] = sign * spec_tm[starts[b] + w, source channel of c, f] (sign = XOR of the sign bit), then the time masks
    (every channel) and the frequency masks (channels < freq_channels) set elements to mask_value; rows past the timeline
    stay zero and unmasked; labels are permuted and never masked."""
    spec_tm = np.ascontiguousarray(spec_tm, dtype=np.float32)
    total, C, bins = spec_tm.shape
    freq_channels = C if freq_channels is None else freq_channels
    B = len(starts)
    spec = np.zeros((B, window, C, bins), dtype=np.float32)
    mask = np.zeros((B, window, I * J), dtype=np.uint16)
    bits = spec_tm.view(np.uint32)
    fill = np.float32(mask_value)
    for b in range(B):
        row = [int(v) for v in params[b]]
        p = row[0]
        n = max(0, min(window, total - int(starts[b])))
        s = int(starts[b])
        if n == 0:
            continue
        for c in range(C):
            entry = int(channel_table[p][c]) if channel_table is not None else c
            got = bits[s:s + n, entry & 0x7f].copy()
            if entry & 0x80:
                got ^= np.uint32(0x80000000)
            spec[b, :n, c] = got.view(np.float32)
        for t0, tl in ((row[1], row[2]), (row[3], row[4])):
            spec[b, t0:min(t0 + tl, n)] = fill
        for f0, fl in ((row[5], row[6]), (row[7], row[8])):
            spec[b, :n, :freq_channels, f0:f0 + fl] = fill
        mask[b, :n] = permute_cells(mask_tm[s:s + n], p, I, J)
    return spec, mask
