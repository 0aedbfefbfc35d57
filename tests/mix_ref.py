"""numpy / float64 restatement of the two-window mix of the device gather, independent of
seld_augment.py and of csrc/mix.hip: the packed partner table, the three row cases, the power mix with the floor rule, the
intensity mix, the label OR, the order of operations -- and the band-limited plane-wave clips on which the power-domain
mix is EXACT (two recordings that share no frequency band have no cross term).

Window b is operand ``a`` (start starts[b], pattern params[b][0]); its partner, if any, is (sb, pb, g) from partners[b].
Per output frame w:
    row starts[b] + w outside the timeline          -> a zero row, features and labels
    no partner, or row sb + w outside the timeline  -> the signed channel copy / cell permutation of operand a alone
    otherwise                                       -> log-mel:   power_to_db(P_a + g P_b), P = 10^(x/10), P = 0 where x <= -100
                                                       intensity: (E_a IV_a + g E_b IV_b) / (E_a + g E_b), 0 where that is 0/0,
                                                                  E = P_W + (P_X + P_Y + P_Z) / 3 of the operand
                                                       labels:    perm_pa(mask[starts[b] + w]) | perm_pb(mask[sb + w])
then x * scale + shift where given, then the time / frequency masks of row a; labels are never masked."""
import numpy as np
import torch

import augment_ref
import rotate_ref
from oracle import features as ofeat

AMIN = 1e-10                                # power_to_db's floor: 10 log10(max(p, AMIN)), exactly -100 dB at or below it
FLOOR_DB = -100.0
PASS_BANDS = ((300.0, 3000.0), (5000.0, 9000.0))        # Hz: clips of even / odd index
MARGIN_HZ = 200.0
LISTED_BANDS = tuple(range(12, 35)) + tuple(range(48, 57))     # mel bands whose filter lies >= 200 Hz inside a pass band


# ------------------------------------------------------------------------------------------ the partner table

def pack_partners(starts_b, patterns_b, gains):
    """int64 [B, 2]: row b = (sb, fp32 bits of g in bits 0..31 | pb in bits 32..35)."""
    bits = np.asarray(gains, dtype=np.float32).view(np.uint32).astype(np.int64)
    out = np.empty((len(bits), 2), dtype=np.int64)
    out[:, 0] = np.asarray(starts_b, dtype=np.int64)
    out[:, 1] = bits | (np.asarray(patterns_b, dtype=np.int64) << 32)
    return out


def unpack_partner(row):
    """(sb, g as a Python float, pb, has a partner) of one row, whatever it holds: the pattern is bits 32..35 and nothing
    else, a partner exists iff g is a finite value > 0."""
    word = int(row[1]) & 0xFFFFFFFFFFFFFFFF
    g = float(np.asarray([word & 0xFFFFFFFF], dtype=np.uint32).view(np.float32)[0])
    return int(row[0]), g, (word >> 32) & 15, bool(np.isfinite(g) and g > 0.0)


def channel_table(channels, order="WYZX"):
    """uint8 [16, channels]: source channel | 0x80 when negated, derived from augment_ref.field_transformed on the unit
    vectors; identity rows unless channels is 4 (log-mel W + XYZ) or 7 (+ the three intensity vectors)."""
    table = np.tile(np.arange(channels, dtype=np.uint8), (16, 1))
    if channels not in (4, 7):
        return table
    basis = np.eye(3)
    for p in range(16):
        for letter, vec in zip("XYZ", augment_ref.field_transformed(basis[0], basis[1], basis[2], p)):
            src = int(np.argmax(np.abs(vec)))
            c, sc = order.index(letter), order.index("XYZ"[src])
            table[p, c] = sc
            if channels == 7:
                table[p, 3 + c] = (3 + sc) | (0x80 if vec[src] < 0 else 0)
    return table


# ------------------------------------------------------------------------------------------ the mix itself

def db_to_power(x):
    x = np.asarray(x, dtype=np.float64)
    return np.where(x <= FLOOR_DB, 0.0, 10.0 ** (x / 10.0))


def power_to_db(p):
    p = np.asarray(p, dtype=np.float64)
    return np.where(p > AMIN, 10.0 * np.log10(np.maximum(p, AMIN)), FLOOR_DB)


def mix_values(xa, xb, g, iv_channels=0):
    """The mix of two operands already transformed, channel axis first: xa, xb [C, ...] float64 (dB for the first
    C - iv_channels channels, intensity vectors for the rest).  Returns (out, power): the mixed values and the float64
    power P_a + g P_b of the log-mel channels."""
    xa, xb = np.asarray(xa, dtype=np.float64), np.asarray(xb, dtype=np.float64)
    n_mel = xa.shape[0] - iv_channels
    pa, pb = db_to_power(xa[:n_mel]), db_to_power(xb[:n_mel])
    power = pa + g * pb
    out = np.empty_like(xa)
    out[:n_mel] = power_to_db(power)
    if iv_channels:
        assert n_mel == 4 and iv_channels == 3
        ea = pa[0] + (pa[1] + pa[2] + pa[3]) / 3.0
        eb = g * (pb[0] + (pb[1] + pb[2] + pb[3]) / 3.0)
        den = ea + eb
        with np.errstate(divide="ignore", invalid="ignore"):
            out[n_mel:] = np.where(den > 0, (ea * xa[n_mel:] + eb * xb[n_mel:]) / den, 0.0)
    return out, power


def _signed(rows, entries):
    """rows float64 [n, C, 64] -> the signed channel copy a channel-table row prescribes."""
    out = np.empty_like(rows)
    for c, entry in enumerate(entries):
        src = rows[:, int(entry) & 0x7f]
        out[:, c] = -src if int(entry) & 0x80 else src
    return out


def gather(spec_tm, mask_tm, starts, params, partners, window, table, iv_channels=0, freq_channels=None, mask_value=0.0,
           scale=None, shift=None, I=18, J=36):
    """What the mixing pair writes and what bounds it, from the device's own fp32 timeline.  Returns
    (want float64 [B, window, C, 64]; tol float64, same shape; computed bool, same shape -- False: a copied, masked or zero
    element; floor_ok bool -- the -100 dB floor is also accepted; labels uint16 [B, window, I*J]; mixed bool [B, window]).
    Bounds of a computed element (fp32 arithmetic on fp32 inputs):
      log-mel  1e-5 + 4.343 2^-24 (0.2303 max(|x_a|, |x_b + 10 log10 g|) + 6) dB: the rounding of x log2(10) / 10 scales with
               |x|, a few ulp for exp2, the fused multiply-add and the product, power_to_db's own 1e-5;
      intensity  64 2^-24 (|IV_a| + |IV_b|): each weight carries that relative error at |x| <= 100, above and below the bar.
    With scale / shift the bound of v becomes |scale| tol + 2^-24 |v scale + shift|: the map's slope and its one rounding."""
    spec_tm = np.ascontiguousarray(spec_tm, dtype=np.float32)
    total, C, bins = spec_tm.shape
    freq_channels = C if freq_channels is None else freq_channels
    n_mel = C - iv_channels
    B = len(starts)
    want = np.zeros((B, window, C, bins))
    tol = np.zeros_like(want)
    computed = np.zeros(want.shape, dtype=bool)
    floor_ok = np.zeros(want.shape, dtype=bool)
    labels = np.zeros((B, window, I * J), dtype=np.uint16)
    mixed = np.zeros((B, window), dtype=bool)
    fill = float(np.float32(mask_value))
    ulp = 2.0 ** -24
    for b in range(B):
        row = [int(v) for v in params[b]]
        pa = row[0] & 15
        sa = int(starts[b])
        sb, g, pb, on = unpack_partner(partners[b])
        live = [w for w in range(window) if 0 <= sa + w < total]
        if not live:
            continue
        wa = np.asarray(live)
        xa = _signed(spec_tm[sa + wa].astype(np.float64), table[pa])
        want[b, wa] = xa
        labels[b, wa] = augment_ref.permute_cells(mask_tm[sa + wa], pa, I, J)
        both = np.asarray([w for w in live if on and 0 <= sb + w < total], dtype=np.int64)
        if len(both):
            mixed[b, both] = True
            xa = _signed(spec_tm[sa + both].astype(np.float64), table[pa]).transpose(1, 0, 2)      # [C, n, 64]
            xb = _signed(spec_tm[sb + both].astype(np.float64), table[pb]).transpose(1, 0, 2)
            out, power = mix_values(xa, xb, g, iv_channels)
            want[b, both] = out.transpose(1, 0, 2)
            level = np.maximum(np.abs(xa[:n_mel]), np.abs(xb[:n_mel] + 10.0 * np.log10(g)))
            t = np.empty_like(out)
            t[:n_mel] = 1e-5 + 4.343 * ulp * (0.2303 * level + 6.0)
            t[n_mel:] = 64.0 * ulp * (np.abs(xa[n_mel:]) + np.abs(xb[n_mel:]))
            tol[b, both] = t.transpose(1, 0, 2)
            computed[b, both] = True
            floor_ok[b, both, :n_mel] = (power < 2e-10).transpose(1, 0, 2)
            labels[b, both] |= augment_ref.permute_cells(mask_tm[sb + both], pb, I, J)
        if scale is not None:
            sc, sh = np.asarray(scale, dtype=np.float64), np.asarray(shift, dtype=np.float64)
            want[b, wa] = want[b, wa] * sc + sh
            tol[b, wa] = np.where(computed[b, wa], tol[b, wa] * np.abs(sc) + ulp * np.abs(want[b, wa]), 0.0)
        for t0, tl in ((row[1], row[2]), (row[3], row[4])):
            for w in range(max(t0, 0), min(t0 + tl, window)):
                if 0 <= sa + w < total:
                    want[b, w], tol[b, w], floor_ok[b, w], computed[b, w] = fill, 0.0, False, False
        for f0, fl in ((row[5], row[6]), (row[7], row[8])):
            want[b, wa, :freq_channels, f0:f0 + fl] = fill
            tol[b, wa, :freq_channels, f0:f0 + fl] = 0.0
            floor_ok[b, wa, :freq_channels, f0:f0 + fl] = False
            computed[b, wa, :freq_channels, f0:f0 + fl] = False
    return want, tol, computed, floor_ok, labels, mixed


# ------------------------------------------------------------------------------------------ band-limited clips

def band_limited_clip(order="WYZX", index=0):
    """float64 [4, L]: ``rotate_ref.plane_wave_clip(order, index)`` through a whole-clip FFT brick wall, 300 - 3 000 Hz for
    an even index and 5 000 - 9 000 Hz for an odd one.  Clips of different parity share no frequency, so the power of their
    sum is the sum of their powers in every STFT bin away from the clip's (reflect-padded) ends."""
    x = rotate_ref.plane_wave_clip(order, index).numpy().astype(np.float64)
    lo, hi = PASS_BANDS[index % 2]
    spectrum = np.fft.rfft(x, axis=-1)
    f = np.fft.rfftfreq(x.shape[-1], 1.0 / ofeat.SR)
    spectrum[:, (f < lo) | (f > hi)] = 0.0
    return np.fft.irfft(spectrum, n=x.shape[-1], axis=-1)


def band_limited_clip_f32(order="WYZX", index=0):
    return torch.from_numpy(band_limited_clip(order, index).astype(np.float32))


def bands_inside_a_pass_band(margin_hz=MARGIN_HZ):
    """The mel bands whose filter support lies at least ``margin_hz`` inside one of PASS_BANDS (LISTED_BANDS, derived)."""
    fb = ofeat.mel_filterbank_htk().numpy()                                        # [481, 64]
    hz = np.arange(fb.shape[0]) * (ofeat.SR / 2.0 / (fb.shape[0] - 1))
    keep = []
    for band in range(fb.shape[1]):
        on = np.nonzero(fb[:, band])[0]
        if len(on) and any(hz[on[0]] >= lo + margin_hz and hz[on[-1]] <= hi - margin_hz for lo, hi in PASS_BANDS):
            keep.append(band)
    return tuple(keep)


def clip_rows(index):
    """Metadata of clip ``index``: ``rotate_ref.clip_rows()`` with the classes moved up by ``index`` and the azimuths by
    40 degrees x index (still off the cell edges), so two clips' labels differ and their union is not either of them."""
    rows = rotate_ref.clip_rows()
    rows[:, 1] += index
    rows[:, 3] = (rows[:, 3] + 40 * index + 180) % 360 - 180
    assert (rows[:, 3] % 10 != 0).all() and (rows[:, 1] < 13).all()
    return rows


def united_rows(rows_a, rows_b):
    """The metadata of two recordings played at once: every row of both, the second one's source numbers moved past the
    first one's, in frame order."""
    rows_b = np.array(rows_b, dtype=np.int64, copy=True)
    rows_b[:, 2] += int(np.asarray(rows_a)[:, 2].max()) + 1
    both = np.concatenate([np.asarray(rows_a, dtype=np.int64), rows_b])
    return both[np.argsort(both[:, 0], kind="stable")]
