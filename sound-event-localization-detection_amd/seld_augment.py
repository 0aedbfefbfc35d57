"""Training augmentation of the device feed: the tables and the per-window draw behind ``csrc/augment.hip``
(DESIGN.md section 11).  Host-side integer work only; the batches themselves are transformed by the gather kernels.

Spatial pattern ``p`` in 0..15, applied to a whole window (``p = 0`` is the identity):

    mirror first     m = p >> 3         az -> -az                 Y -> -Y
    then rotate      k = (p >> 1) & 3   az -> az + 90 k           k = 1: X' = -Y, Y' = X;  2: X' = -X, Y' = -Y;  3: X' = Y, Y' = -X
    then flip        e = p & 1          el -> -el                 Z -> -Z

with X = cos az cos el, Y = sin az cos el, Z = sin el; W never changes.  These are the 16 sign-and-swap transforms of the
first-order-Ambisonics channels ("audio channel swapping"); on the 10-degree grid each one is an exact permutation of the
cells, so features AND labels of the transformed sound field are gathers of the stored ones.

Parameter row of one window (int32 x 12, ``include/seld_hip.h``):
    [0] pattern   [1] [2] [3] [4] two time masks (first frame, length)   [5] [6] [7] [8] two frequency masks
    [9] azimuth step r   [10] [11] 0

Rotation in azimuth steps (``csrc/rotate.hip``): on the I x J grid a rotation about the vertical axis by
a multiple of one cell (10 degrees) is still an exact cyclic shift of the label cells.  A window's transform is then
mirror m, s = (k J/4 + r) mod J cells of azimuth (phi = 2 pi s / J), elevation flip e: 2 x J x 2 = 144 transforms.

Microphone arrays (``csrc/micswap.hip``): with the microphone positions known (``Config.MIC_POSITIONS``),
every pattern that maps the array onto itself is an exact permutation of the recording's channels -- ``mic_permutations``
-- and the label-cell permutation above applies unchanged.  ``draw`` then picks among the array's valid patterns only.
"""
from __future__ import annotations

import math

import numpy as np

PARAM_INTS = 12                   # SELD_AUGMENT_PARAM_INTS; seld_native takes both from here
PATTERNS = 16                     # SELD_AUGMENT_PATTERNS
N_BINS = 64
NEGATE = 0x80                     # channel-table flag: the output channel is MINUS its source channel

STEP = 9                          # parameter-row slot of the azimuth step r
MAX_STEPS = 72                    # SELD_ROTATE_MAX_STEPS

MIC_MIN, MIC_MAX = 2, 8          # microphones the array gather takes (csrc/micswap.hip)
MIC_MATCH_TOLERANCE = 1e-3        # a moved microphone matches a position within this share of the largest |r_j|
MIC_FEATURE_SETS = ("logmel", "logmel_gcc", "logmel_nipd")      # the feature sets with a defined swap on an array
# (azimuth, elevation) in degrees and radius in metres of the preset arrays
MIC_PRESETS = {"tetra_starss": (((45.0, 35.0), (-45.0, -35.0), (135.0, -35.0), (-135.0, 35.0)), 0.042)}

SPECTRAL_PARAM_INTS = 12          # SELD_SPECTRAL_PARAM_INTS: the spectral row of the in-place stage (csrc/spectral.hip)
SPECTRAL_CURVE = 1                # flag bit 0 of slot [1]: the window has a gain curve
FILTER_TYPES = ("linear", "step")

SPECTRAL_SWITCHES = ("AUGMENT_FREQ_SHIFT_MAX", "AUGMENT_LEVEL_DB", "AUGMENT_FILTER_PROB", "AUGMENT_CUTOUTS")
SWITCHES = ("AUGMENT_SPATIAL", "AUGMENT_TIME_MASKS", "AUGMENT_FREQ_MASKS", "AUGMENT_ROTATE", "AUGMENT_MIX_PROB") + SPECTRAL_SWITCHES


def decode(p: int):
    """pattern -> (mirror, quarter turns, elevation flip)."""
    if not 0 <= int(p) < PATTERNS:
        raise ValueError(f"spatial pattern {p} outside 0..15")
    return (int(p) >> 3) & 1, (int(p) >> 1) & 3, int(p) & 1


def axis_map(p: int):
    """{'X' | 'Y' | 'Z': (source axis, sign)}: the transformed field's axis is sign * the original field's source axis."""
    m, k, e = decode(p)
    x, y = ("X", 1), ("Y", -1 if m else 1)
    neg = lambda a: (a[0], -a[1])
    x, y = ((x, y), (neg(y), x), (neg(x), neg(y)), (y, neg(x)))[k]
    return {"X": x, "Y": y, "Z": ("Z", -1 if e else 1)}


def check_channel_order(order: str) -> str:
    order = str(order).upper()
    if len(order) != 4 or order[0] != "W" or sorted(order[1:]) != ["X", "Y", "Z"]:
        raise ValueError(f"FOA_CHANNEL_ORDER must be 'WYZX' (STARSS / DCASE recordings) or 'WXYZ', got {order!r}")
    return order


def spatial_supported(feature_set: str, n_channels: int) -> bool:
    """Channel swapping is defined for 4-channel FOA input only: 'logmel' with 4 channels and 'logmel_iv' (4 + 3)."""
    return (feature_set == "logmel" and n_channels == 4) or (feature_set == "logmel_iv" and n_channels == 7)


def channel_table(feature_set: str, n_channels: int, order: str = "WYZX") -> np.ndarray:
    """uint8 [16, n_channels]: entry [p, c] = source channel of output channel c under pattern p, | NEGATE when the output is
    minus the source.  A log-mel channel takes the log-mel of its source channel (a power: the sign drops out); an
    intensity-vector channel (4 + n pairs W with input channel 1 + n) takes the SIGNED channel of its source axis.  Feature
    sets without a defined swap get identity rows (the masks still apply)."""
    table = np.tile(np.arange(n_channels, dtype=np.uint8), (PATTERNS, 1))
    if not spatial_supported(feature_set, n_channels):
        return table
    order = check_channel_order(order)
    for p in range(PATTERNS):
        mp = axis_map(p)
        for c in range(1, 4):
            src_axis, sign = mp[order[c]]
            sc = order.index(src_axis)
            table[p, c] = sc
            if n_channels == 7:
                table[p, 3 + c] = (3 + sc) | (NEGATE if sign < 0 else 0)
    return table


def mix_supported(feature_set: str) -> bool:
    """Two windows can be mixed on the stored features where these are powers (log-mel) or power-normalised intensities:
    'logmel' with any channel count and 'logmel_iv' (DESIGN.md section 24)."""
    return feature_set in ("logmel", "logmel_iv")


def mix_iv_channels(feature_set: str, n_channels: int) -> int:
    """The ``iv_channels`` argument of the mixing gather: 3 for 'logmel_iv' (channels 4..6), else 0."""
    return 3 if feature_set == "logmel_iv" and int(n_channels) == 7 else 0


def freq_mask_channels(feature_set: str, n_channels: int) -> int:
    """Frequency masks apply to channels [0, this): log-mel and intensity vectors have a 64-bin FREQUENCY axis, the 64-wide
    axis of a GCC-PHAT channel is lags.  Every other set gets all its channels: that is what 'logmel_nipd' wants, whose
    2C - 1 channels (C log-mel, C - 1 mel-band NIPD) all lie on the mel axis."""
    if feature_set == "logmel_gcc":                     # C + C(C-1)/2 channels: the first C are log-mel
        c = int(round((np.sqrt(8 * n_channels + 1) - 1) / 2))
        return c if c * (c + 1) // 2 == n_channels else 0
    return n_channels


def logmel_channels(feature_set: str, n_channels: int) -> int:
    """The leading channels that are log-mel in dB -- the ones a gain curve of the spectral stage is added to (DESIGN.md
    section 26): every channel of 'logmel', 4 of 'logmel_iv', the microphones of 'logmel_gcc' / 'logmel_nipd'; 0 for a
    channel count that fits no such set."""
    if feature_set == "logmel":
        return int(n_channels)
    if feature_set == "logmel_iv":
        return 4
    return mic_count(feature_set, n_channels)


def cell_dest(p: int, I: int = 18, J: int = 36) -> np.ndarray:
    """int64 [I*J]: the cell a set cell moves TO: (i, j) -> (e ? I-1-i : i, ((m ? J-1-j : j) + k J/4) mod J)."""
    m, k, e = decode(p)
    return cell_dest_rot(m, total_step(k, 0, J), e, I, J)


def cell_source(p: int, I: int = 18, J: int = 36) -> np.ndarray:
    """int64 [I*J]: the gather form, out[..., c] = in[..., cell_source[c]] (the inverse permutation of ``cell_dest``)."""
    dest = cell_dest(p, I, J)
    src = np.empty_like(dest)
    src[dest] = np.arange(I * J, dtype=np.int64)
    return src


# ------------------------------------------------------------------------------------------ rotation in azimuth steps

def total_step(k: int, r: int, J: int = 36) -> int:
    """Cells of azimuth a window is turned by: k quarter turns of the pattern plus the step r, modulo J."""
    if J % 4:
        raise ValueError("a quarter turn is a whole number of cells only when J % 4 == 0")
    return (int(k) * (J // 4) + int(r)) % J


def rotation_table(J: int = 36) -> np.ndarray:
    """float32 [J, 2]: (cos, sin) of 2 pi s / J, evaluated in double precision and rounded once; exactly 0 / +-1 at the quarter
    turns.  The table ``seld_window_gather_rotate`` builds for its kernel."""
    if J % 4 or not 4 <= J <= MAX_STEPS:
        raise ValueError(f"rotation steps: J must be a multiple of 4 in 4..{MAX_STEPS}, got {J}")
    table = np.zeros((J, 2), dtype=np.float32)
    for s in range(J):
        if (4 * s) % J == 0:
            table[s] = ((1, 0), (0, 1), (-1, 0), (0, -1))[4 * s // J]
        else:
            phi = 2.0 * math.pi * s / J
            table[s] = (math.cos(phi), math.sin(phi))
    return table


def cell_dest_rot(m: int, s: int, e: int, I: int = 18, J: int = 36) -> np.ndarray:
    """int64 [I*J]: the cell a set cell moves TO under mirror m, then s cells of azimuth, then elevation flip e:
    (i, j) -> (e ? I-1-i : i, ((m ? J-1-j : j) + s) mod J).  ``cell_dest(p)`` is the case s = k J/4."""
    i, j = np.divmod(np.arange(I * J, dtype=np.int64), J)
    i2 = I - 1 - i if e else i
    j2 = ((J - 1 - j if m else j) + int(s)) % J
    return i2 * J + j2


def cell_source_rot(m: int, s: int, e: int, I: int = 18, J: int = 36) -> np.ndarray:
    """int64 [I*J]: the gather form, out[..., c] = in[..., cell_source_rot[c]] (the inverse of ``cell_dest_rot``)."""
    dest = cell_dest_rot(m, s, e, I, J)
    src = np.empty_like(dest)
    src[dest] = np.arange(I * J, dtype=np.int64)
    return src


# ------------------------------------------------------------------------------------------ microphone arrays

def mic_positions(spec):
    """Microphone positions as float64 [C, 3] (x, y, z in metres, the DOA frame of the labels: x towards azimuth 0 /
    elevation 0, y towards azimuth +90 degrees, z up) from a Config.MIC_POSITIONS value: None stays None (no array: FOA
    rules), the preset name 'tetra_starss' (the STARSS22 tetrahedron), or C rows of (x, y, z)."""
    if spec is None:
        return None
    if isinstance(spec, str):
        if spec not in MIC_PRESETS:
            raise ValueError(f"MIC_POSITIONS: unknown preset {spec!r}; the presets are {sorted(MIC_PRESETS)}")
        angles, radius = MIC_PRESETS[spec]
        az, el = np.radians(np.asarray(angles, dtype=np.float64)).T
        return radius * np.stack([np.cos(az) * np.cos(el), np.sin(az) * np.cos(el), np.sin(el)], axis=1)
    try:
        pos = np.array(spec, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError("MIC_POSITIONS must be None, a preset name or rows of (x, y, z) in metres") from None
    if pos.ndim != 2 or pos.shape[1] != 3:
        raise ValueError(f"MIC_POSITIONS must be rows of (x, y, z) in metres, got shape {pos.shape}")
    if pos.shape[0] < 2:
        raise ValueError(f"MIC_POSITIONS: an array has at least 2 microphones, got {pos.shape[0]}")
    if not np.isfinite(pos).all():
        raise ValueError("MIC_POSITIONS: positions must be finite")
    scale = float(np.sqrt((pos * pos).sum(axis=1)).max())
    gaps = np.sqrt(((pos[:, None, :] - pos[None, :, :]) ** 2).sum(axis=2)) + np.eye(len(pos)) * (scale + 1.0)
    if gaps.min() <= MIC_MATCH_TOLERANCE * scale:
        raise ValueError("MIC_POSITIONS: two microphones share a position")
    return pos


def pattern_matrix(p: int) -> np.ndarray:
    """float64 [3, 3]: T_p, the orthogonal map of pattern p on a direction (x, y, z): mirror y -> -y, then k quarter turns
    (x, y) -> (-y, x), then flip z -> -z."""
    m, k, e = decode(p)
    mirror = np.diag([1.0, -1.0 if m else 1.0, 1.0])
    turn = np.linalg.matrix_power(np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]]), k)
    flip = np.diag([1.0, 1.0, -1.0 if e else 1.0])
    return flip @ turn @ mirror


def mic_permutations(positions) -> np.ndarray:
    """int8 [16, C]: row p = sigma_p with r[sigma_p(j)] = T_p^-1 r[j] when pattern p maps the array onto itself (every point
    matched exactly once, within MIC_MATCH_TOLERANCE of the largest |r_j|), else all -1.  The transformed scene's channel j
    is the recording's channel sigma_p(j)."""
    pos = mic_positions(positions)
    if pos is None:
        raise ValueError("mic_permutations: no microphone positions")
    n = len(pos)
    tolerance = MIC_MATCH_TOLERANCE * float(np.sqrt((pos * pos).sum(axis=1)).max())
    table = np.full((PATTERNS, n), -1, dtype=np.int8)
    for p in range(PATTERNS):
        moved = pos @ pattern_matrix(p)                             # rows T_p^T r_j = T_p^-1 r_j
        gaps = np.sqrt(((moved[:, None, :] - pos[None, :, :]) ** 2).sum(axis=2))
        sigma = gaps.argmin(axis=1)
        if (gaps[np.arange(n), sigma] <= tolerance).all() and len(set(sigma.tolist())) == n:
            table[p] = sigma
    return table


def mic_valid_patterns(positions) -> tuple:
    """The patterns that are symmetries of the array, ascending; 0 is always one."""
    return tuple(int(p) for p in np.flatnonzero(mic_permutations(positions)[:, 0] >= 0))


def mic_channel_table(positions) -> np.ndarray:
    """uint8 [16, C] for 'logmel' on an array: the channel table of ``seld_window_gather_augment`` whose row p is sigma_p
    (log-mel channels are copied, never negated); rows of patterns that are no symmetry are the identity."""
    perm = mic_permutations(positions)
    table = np.tile(np.arange(perm.shape[1], dtype=np.uint8), (PATTERNS, 1))
    valid = perm[:, 0] >= 0
    table[valid] = perm[valid].astype(np.uint8)
    return table


def mic_count(feature_set: str, n_channels: int) -> int:
    """Microphones behind ``n_channels`` feature channels: C for 'logmel', C + C(C-1)/2 for 'logmel_gcc', 2C - 1 for
    'logmel_nipd'; 0 when the count fits no array."""
    n = int(n_channels)
    if feature_set == "logmel":
        return n
    if feature_set == "logmel_gcc":
        c = int(round((math.sqrt(8 * n + 1) - 1) / 2))
        return c if c * (c + 1) // 2 == n else 0
    if feature_set == "logmel_nipd":
        return (n + 1) // 2 if n % 2 == 1 else 0
    return 0


def _array_of(cfg, array):
    """The array an entry point works with: the one it was handed, else the Config's."""
    return mic_positions(array if array is not None else getattr(cfg, "MIC_POSITIONS", None))


def _check_array_features(array, feature_set, n_channels):
    if feature_set not in MIC_FEATURE_SETS:
        raise ValueError(
            f"MIC_POSITIONS describes a microphone array: its channel swap is defined for FEATURE_SET 'logmel', "
            f"'logmel_gcc' and 'logmel_nipd', not for {feature_set!r} (first-order-Ambisonics features have no microphone "
            f"positions; leave MIC_POSITIONS at None for them)")
    if n_channels is not None and mic_count(feature_set, int(n_channels)) != len(array):
        raise ValueError(
            f"MIC_POSITIONS holds {len(array)} microphones, FEATURE_SET={feature_set!r} with {n_channels} feature channels "
            f"comes from {mic_count(feature_set, int(n_channels))}")


# ------------------------------------------------------------------------------------------ configuration

def settings(cfg):
    """The augmentation switches of a Config as a plain dict (missing attributes = off)."""
    return {
        "spatial": bool(getattr(cfg, "AUGMENT_SPATIAL", False)),
        "rotate": bool(getattr(cfg, "AUGMENT_ROTATE", False)),
        "time_masks": int(getattr(cfg, "AUGMENT_TIME_MASKS", 0)),
        "time_max": int(getattr(cfg, "AUGMENT_TIME_MASK_MAX", 0)),
        "freq_masks": int(getattr(cfg, "AUGMENT_FREQ_MASKS", 0)),
        "freq_max": int(getattr(cfg, "AUGMENT_FREQ_MASK_MAX", 0)),
        "mask_value": float(getattr(cfg, "AUGMENT_MASK_VALUE", 0.0)),
        "order": str(getattr(cfg, "FOA_CHANNEL_ORDER", "WYZX")),
        "mix_prob": float(getattr(cfg, "AUGMENT_MIX_PROB", 0.0)),
        "mix_gain_db": float(getattr(cfg, "AUGMENT_MIX_GAIN_DB", 6.0)),
        # the in-place spectral stage (csrc/spectral.hip)
        "freq_shift_max": int(getattr(cfg, "AUGMENT_FREQ_SHIFT_MAX", 0)),
        "level_db": float(getattr(cfg, "AUGMENT_LEVEL_DB", 0.0)),
        "filter_prob": float(getattr(cfg, "AUGMENT_FILTER_PROB", 0.0)),
        "filter_db": float(getattr(cfg, "AUGMENT_FILTER_DB", 6.0)),
        "filter_bands": tuple(getattr(cfg, "AUGMENT_FILTER_BANDS", (3, 6))),
        "filter_type": str(getattr(cfg, "AUGMENT_FILTER_TYPE", "linear")),
        "cutouts": int(getattr(cfg, "AUGMENT_CUTOUTS", 0)),
        "cutout_time_max": int(getattr(cfg, "AUGMENT_CUTOUT_TIME_MAX", 0)),
        "cutout_freq_max": int(getattr(cfg, "AUGMENT_CUTOUT_FREQ_MAX", 0)),
    }


def spectral_enabled(cfg) -> bool:
    """A switch of the in-place spectral stage is on: the feed then draws spectral rows (``draw_spectral``)."""
    s = settings(cfg)
    return s["freq_shift_max"] != 0 or s["level_db"] != 0 or s["filter_prob"] != 0 or s["cutouts"] != 0


def enabled(cfg) -> bool:
    s = settings(cfg)
    return (s["spatial"] or s["rotate"] or s["time_masks"] > 0 or s["freq_masks"] > 0 or s["mix_prob"] > 0
            or spectral_enabled(cfg))


PCEN_SETTINGS = ("PCEN", "PCEN_TIME_CONSTANT", "PCEN_GAIN", "PCEN_BIAS", "PCEN_POWER", "PCEN_EPS")
# the switches that are defined on dB or power values and so have no meaning on PCEN values, with how each counts as on
PCEN_EXCLUDES = (("AUGMENT_MIX_PROB", "mix_prob"), ("AUGMENT_ROTATE", "rotate"), ("AUGMENT_LEVEL_DB", "level_db"),
                 ("AUGMENT_FILTER_PROB", "filter_prob"))


def pcen_settings(cfg):
    """The per-channel energy normalisation a Config asks for: None with Config.PCEN off, else
    {'PCEN_TIME_CONSTANT', 'PCEN_GAIN', 'PCEN_BIAS', 'PCEN_POWER', 'PCEN_EPS': float}, checked against the ranges the
    kernel takes (ValueError)."""
    if not bool(getattr(cfg, "PCEN", False)):
        return None
    p = {name: float(getattr(cfg, name)) for name in PCEN_SETTINGS[1:]}
    if not all(np.isfinite(v) for v in p.values()):
        raise ValueError(f"the PCEN settings must be finite, got {p}")
    if not p["PCEN_TIME_CONSTANT"] > 0:
        raise ValueError(f"PCEN_TIME_CONSTANT must be a positive time in seconds, got {p['PCEN_TIME_CONSTANT']}")
    if not 0.0 <= p["PCEN_GAIN"] <= 1.0:
        raise ValueError(f"PCEN_GAIN must be in [0, 1], got {p['PCEN_GAIN']}")
    if not 0.0 < p["PCEN_POWER"] <= 1.0:
        raise ValueError(f"PCEN_POWER must be in (0, 1], got {p['PCEN_POWER']}")
    if not (p["PCEN_BIAS"] > 0 and p["PCEN_EPS"] > 0):
        raise ValueError(f"PCEN_BIAS and PCEN_EPS must be positive, got {p['PCEN_BIAS']} and {p['PCEN_EPS']}")
    return p


def check_settings(cfg, feature_set: str | None = None, n_channels: int | None = None, array=None, pcen: bool | None = None):
    """Raise ValueError for switches outside their range or a spatial swap the feature set does not define.  ``array``:
    microphone positions (``mic_positions``; None reads Config.MIC_POSITIONS) -- with them the spatial rules are those of
    the array in place of the FOA ones.  ``pcen``: the features hold PCEN values (None reads
    Config.PCEN) -- the switches defined on dB or power values are then refused."""
    s = settings(cfg)
    array = _array_of(cfg, array)
    if bool(getattr(cfg, "PCEN", False)) if pcen is None else pcen:
        for name, key in PCEN_EXCLUDES:
            if s[key]:
                raise ValueError(
                    f"{name} cannot be combined with PCEN: it is defined on the log-mel channels' dB or power values (powers "
                    f"add, a level is a dB offset, the rotation terms are mel powers), and with PCEN on those channels hold "
                    f"normalised values.  Switch one of them off (channel swaps, masks, cutout, frequency shift, "
                    f"standardisation and balanced sampling commute with a per-channel transform and stay allowed)")
    for key in ("time_masks", "freq_masks"):
        if not 0 <= s[key] <= 2:
            raise ValueError(f"AUGMENT_{key.upper()} must be 0, 1 or 2, got {s[key]}")
    if s["time_max"] < 0 or s["freq_max"] < 0:
        raise ValueError("AUGMENT_TIME_MASK_MAX / AUGMENT_FREQ_MASK_MAX must not be negative")
    if not np.isfinite(s["mask_value"]):
        raise ValueError("AUGMENT_MASK_VALUE must be finite")
    check_channel_order(s["order"])
    if array is not None:
        if feature_set is not None:
            _check_array_features(array, feature_set, n_channels)
        if s["rotate"]:
            raise ValueError("AUGMENT_ROTATE is not defined for a microphone array (MIC_POSITIONS is set): no array is "
                             "symmetric under 10-degree steps; AUGMENT_SPATIAL draws among the array's own symmetries")
        if s["mix_prob"] > 0 and s["spatial"]:
            raise ValueError("AUGMENT_MIX_PROB cannot be combined with AUGMENT_SPATIAL on a microphone array (MIC_POSITIONS is "
                             "set): the partner's pattern is drawn over all 16, not over the array's symmetries")
    foa_rules = array is None and feature_set is not None           # an array has its own rules, above
    if s["spatial"] and foa_rules and not spatial_supported(feature_set, int(n_channels)):
        raise ValueError(
            f"AUGMENT_SPATIAL is defined for 4-channel FOA features ('logmel' with 4 channels, 'logmel_iv'), not for "
            f"FEATURE_SET={feature_set!r} with {n_channels} feature channels: a microphone array's geometry is unknown here, "
            f"so no channel swap is defined (time / frequency masks work for every feature set)")
    if s["rotate"] and foa_rules and not spatial_supported(feature_set, int(n_channels)):
        raise ValueError(
            f"AUGMENT_ROTATE is defined for 4-channel FOA features ('logmel' with 4 channels, 'logmel_iv'), not for "
            f"FEATURE_SET={feature_set!r} with {n_channels} feature channels: a microphone array's geometry is unknown here, "
            f"so no rotation is defined (time / frequency masks work for every feature set)")
    if not 0.0 <= s["mix_prob"] <= 1.0:                 # a NaN fails both comparisons
        raise ValueError(f"AUGMENT_MIX_PROB must be a probability in [0, 1], got {s['mix_prob']}")
    if not (np.isfinite(s["mix_gain_db"]) and s["mix_gain_db"] >= 0):
        raise ValueError(f"AUGMENT_MIX_GAIN_DB must be finite and not negative, got {s['mix_gain_db']}")
    if s["mix_prob"] > 0 and s["rotate"]:
        raise ValueError(
            "AUGMENT_MIX_PROB cannot be combined with AUGMENT_ROTATE: the mixing gather transforms each operand with one of "
            "the 16 sign-and-swap patterns (AUGMENT_SPATIAL) and does not read the rotation terms; switch one of them off")
    if s["mix_prob"] > 0 and feature_set is not None and not mix_supported(feature_set):
        raise ValueError(
            f"AUGMENT_MIX_PROB is defined for power features ('logmel' with any channel count, 'logmel_iv'), not for "
            f"FEATURE_SET={feature_set!r} with {n_channels} feature channels: the powers of two recordings add, the phase cues "
            f"of two sound fields (GCC-PHAT lags, NIPD) do not add in any stored form, so no mix is defined")
    _check_spectral_settings(s)
    return s


def _check_spectral_settings(s):
    """The switches of the in-place spectral stage."""
    if not 0 <= s["freq_shift_max"] <= N_BINS - 1:
        raise ValueError(f"AUGMENT_FREQ_SHIFT_MAX must be 0..{N_BINS - 1} bins, got {s['freq_shift_max']}")
    if not (np.isfinite(s["level_db"]) and s["level_db"] >= 0):
        raise ValueError(f"AUGMENT_LEVEL_DB must be finite and not negative, got {s['level_db']}")
    if not 0.0 <= s["filter_prob"] <= 1.0:              # a NaN fails both comparisons
        raise ValueError(f"AUGMENT_FILTER_PROB must be a probability in [0, 1], got {s['filter_prob']}")
    if not (np.isfinite(s["filter_db"]) and s["filter_db"] >= 0):
        raise ValueError(f"AUGMENT_FILTER_DB must be finite and not negative, got {s['filter_db']}")
    bands = s["filter_bands"]
    if not (len(bands) == 2 and all(isinstance(n, (int, np.integer)) and not isinstance(n, bool) for n in bands)
            and 1 <= bands[0] <= bands[1] <= N_BINS):
        raise ValueError(f"AUGMENT_FILTER_BANDS must be (fewest, most) bands with 1 <= fewest <= most <= {N_BINS}, got {bands}")
    if s["filter_type"] not in FILTER_TYPES:
        raise ValueError(f"AUGMENT_FILTER_TYPE must be 'linear' or 'step', got {s['filter_type']!r}")
    if not 0 <= s["cutouts"] <= 2:
        raise ValueError(f"AUGMENT_CUTOUTS must be 0, 1 or 2, got {s['cutouts']}")
    if s["cutout_time_max"] < 0 or s["cutout_freq_max"] < 0:
        raise ValueError("AUGMENT_CUTOUT_TIME_MAX / AUGMENT_CUTOUT_FREQ_MAX must not be negative")


def identity_rows(n: int) -> np.ndarray:
    return np.zeros((int(n), PARAM_INTS), dtype=np.int32)


# ------------------------------------------------------------------------------------------ test-time augmentation

def tta_patterns(spec, array=None) -> tuple:
    """The pattern list of test-time augmentation from a Config value or a command-line string:
    None, (), 0, False and "" give () (off); "all" the 16 patterns; an iterable of ints or a comma-separated string is
    checked (each in 0..15, no duplicates) and its order kept.  ``array``: microphone positions (``mic_positions``) --
    "all" is then the array's valid patterns (``check_tta`` refuses listed ones that are not)."""
    if spec is None or spec is False or (isinstance(spec, (int, np.integer)) and not isinstance(spec, bool) and spec == 0):
        return ()
    if spec is True:
        raise ValueError("test-time augmentation patterns: True names no list; use 'all' or the patterns")
    if isinstance(spec, str):
        text = spec.strip()
        if text.lower() == "all":
            return tuple(range(PATTERNS)) if array is None else mic_valid_patterns(array)
        if text == "":
            return ()
        try:
            spec = [int(part) for part in text.split(",")]
        except ValueError:
            raise ValueError(f"test-time augmentation patterns must be 'all' or comma-separated integers, got {text!r}") from None
    elif isinstance(spec, (int, np.integer)):
        spec = [spec]
    out = []
    for value in spec:
        if isinstance(value, bool) or not isinstance(value, (int, np.integer)):
            raise ValueError(f"test-time augmentation pattern {value!r} is not an integer")
        decode(value)
        if int(value) in out:
            raise ValueError(f"test-time augmentation pattern {int(value)} is listed twice")
        out.append(int(value))
    return tuple(out)


def tta_rows(p: int, n: int) -> np.ndarray:
    """int32 [n, 12] parameter rows of n windows under spatial pattern p and no masks."""
    decode(p)
    rows = identity_rows(n)
    rows[:, 0] = int(p)
    return rows


def check_tta(patterns, feature_set: str, n_channels: int, array=None):
    """Raise ValueError when a non-empty pattern list meets a feature set without a defined channel swap.  ``array``:
    microphone positions (``mic_positions``) -- the feature set must then be one of the array's and every pattern one of
    its symmetries."""
    array = mic_positions(array)
    if patterns and array is not None:
        _check_array_features(array, feature_set, n_channels)
        valid = mic_valid_patterns(array)
        wrong = [int(p) for p in patterns if int(p) not in valid]
        if wrong:
            raise ValueError(f"test-time augmentation patterns {wrong} are no symmetries of this microphone array; its valid "
                             f"patterns are {list(valid)}")
        return
    if patterns and not spatial_supported(feature_set, int(n_channels)):
        raise ValueError(
            f"test-time augmentation over the spatial patterns is defined for 4-channel FOA features ('logmel' with 4 "
            f"channels, 'logmel_iv'), not for FEATURE_SET={feature_set!r} with {n_channels} feature channels: a microphone "
            f"array's geometry is unknown here, so no channel swap is defined")


def _stream_keys(idx, keys) -> np.ndarray:
    """The per-window generator keys of the three draws: the window indices themselves, or ``keys`` -- one integer per
    window, what a feed that holds a window several times per epoch hands over (class-balanced sampling, DESIGN.md section
    28: each draw's position in the epoch's global order)."""
    if keys is None:
        return idx
    keys = np.asarray(keys, dtype=np.int64).reshape(-1)
    if len(keys) != len(idx):
        raise ValueError(f"keys must hold one integer per window: {len(keys)} for {len(idx)} windows")
    if len(keys) and int(keys.min()) < 0:
        raise ValueError("keys must not be negative")
    return keys


def draw(seed: int, epoch: int, window_indices, cfg, window: int | None = None, bins: int = N_BINS,
         steps: int | None = None, array=None, keys=None) -> np.ndarray:
    """int32 [B, 12] parameter rows for the windows ``window_indices`` (dataset window indices) of ``epoch``.

    A window's row is a function of (seed, epoch, window index) and the switches ONLY -- not of the rank, the batch size
    or the position in the batch -- so N-rank training sees the same augmented windows as one rank, and a window repeated
    by the data-parallel wrap padding gets the same transform both times.  The pattern is uniform over the 16; a mask
    length is a uniform integer in [0, max] (max clipped to the axis), its start uniform over the positions that fit.

    With AUGMENT_ROTATE the spatial part is drawn over the 4 J transforms instead: mirror and elevation flip uniform, no
    quarter turns in the pattern (m << 3 | e), the azimuth step [9] uniform in 0..steps-1 (``steps``: the grid's J, default
    360 // GRID_CELL_DEGREES).  With it off the generator is asked exactly what it was asked before the switch existed.

    With Config.MIC_POSITIONS (a microphone array) AUGMENT_SPATIAL draws uniformly among the array's
    valid patterns, ``valid[rng.integers(0, len(valid))]``; with it None the generator is asked exactly what it was asked
    before arrays existed.  ``array``: the positions to draw for in place of the Config's (a feed hands over its dataset's).

    ``keys``: None, or one integer per window that takes the window index's place in the generator's key (``_stream_keys``);
    left out, the rows are what they were before the argument existed."""
    s = check_settings(cfg, array=array)
    array = _array_of(cfg, array)
    valid = mic_valid_patterns(array) if array is not None and s["spatial"] else None
    if steps is None:
        steps = int(360 // getattr(cfg, "GRID_CELL_DEGREES", 10))
    if window is None:
        window = int(int(cfg.WINDOW_LENGTH) / int(cfg.SPECTROGRAM_HOP_LENGTH))
    idx = np.asarray(window_indices, dtype=np.int64).reshape(-1)
    rows = identity_rows(len(idx))
    if not (s["spatial"] or s["rotate"] or s["time_masks"] or s["freq_masks"]):
        return rows
    for r, i in enumerate(_stream_keys(idx, keys)):
        rng = np.random.default_rng([int(seed), int(epoch), int(i)])
        if s["rotate"]:
            rows[r, 0] = (int(rng.integers(0, 2)) << 3) | int(rng.integers(0, 2))
            rows[r, STEP] = rng.integers(0, int(steps))
        elif valid is not None:
            rows[r, 0] = valid[int(rng.integers(0, len(valid)))]
        elif s["spatial"]:
            rows[r, 0] = rng.integers(0, PATTERNS)
        for first, count, longest, axis in ((1, s["time_masks"], s["time_max"], int(window)),
                                            (5, s["freq_masks"], s["freq_max"], int(bins))):
            for n in range(count):
                length = int(rng.integers(0, min(longest, axis) + 1))
                rows[r, first + 2 * n] = rng.integers(0, axis - length + 1)
                rows[r, first + 2 * n + 1] = length
    return rows


def draw_mix(seed: int, epoch: int, window_indices, cfg, n_windows: int, keys=None):
    """The partners of the windows ``window_indices`` of ``epoch`` for the mixing gathers (csrc/mix.hip):
    (partner int64 [B]: a dataset window index, -1 = none; pattern_b int32 [B]: the partner's spatial pattern;
    gain float32 [B]: its linear power gain, 0 = none).

    A window's triple comes from ``np.random.default_rng([seed, epoch, index, 1])`` -- a stream of its own, so ``draw`` asks
    its generator exactly what it asks without the mix -- always in this order: u = random() (a partner iff
    u < AUGMENT_MIX_PROB), the partner uniform over the ``n_windows`` windows of the dataset, its pattern uniform over the 16
    (used only with AUGMENT_SPATIAL, else 0), its level uniform in +-AUGMENT_MIX_GAIN_DB dB; the gain is 10^(dB / 10)
    evaluated in double precision and rounded once.  Like a parameter row the triple is a function of (seed, epoch, window
    index) only: N ranks see the mixtures of one rank, a wrap-padded repeat gets the same partner.  ``keys``: as in ``draw``
    (the key replaces the index in the generator's key; the partner stays uniform over all ``n_windows`` windows)."""
    s = check_settings(cfg)
    idx = np.asarray(window_indices, dtype=np.int64).reshape(-1)
    partner = np.full(len(idx), -1, dtype=np.int64)
    pattern = np.zeros(len(idx), dtype=np.int32)
    gain = np.zeros(len(idx), dtype=np.float32)
    if not s["mix_prob"] > 0:
        return partner, pattern, gain
    if int(n_windows) <= 0:
        raise ValueError("draw_mix: the dataset has no windows to draw a partner from")
    for r, i in enumerate(_stream_keys(idx, keys)):
        rng = np.random.default_rng([int(seed), int(epoch), int(i), 1])
        u = rng.random()
        other = int(rng.integers(0, int(n_windows)))
        p = int(rng.integers(0, PATTERNS))
        level = float(rng.uniform(-s["mix_gain_db"], s["mix_gain_db"]))
        if u < s["mix_prob"]:
            partner[r], gain[r] = other, np.float32(10.0 ** (level / 10.0))
            pattern[r] = p if s["spatial"] else 0
    return partner, pattern, gain


# ------------------------------------------------------------------------------------------ the in-place spectral stage

def identity_spectral_rows(n: int) -> np.ndarray:
    """int32 [n, 12] spectral rows that change nothing: no shift, no curve, no cutout."""
    return np.zeros((int(n), SPECTRAL_PARAM_INTS), dtype=np.int32)


def _uniform_int(u: float, count: int) -> int:
    """u in [0, 1) -> an integer uniform over 0..count-1 (count >= 1); one draw whatever the count."""
    return min(int(u * count), count - 1)


def filter_curve(rng, s, bins: int = N_BINS) -> np.ndarray:
    """float64 [bins]: one FilterAugment curve from ``rng`` -- n bands, n uniform in AUGMENT_FILTER_BANDS; edges
    0 = e_0 < ... < e_n = bins, the interior ones a sorted sample without replacement from 1..bins-1; 'step': one gain per
    band, 'linear': one gain per edge, interpolated linearly inside each band; gains uniform in +-AUGMENT_FILTER_DB."""
    lo, hi = s["filter_bands"]
    n = int(rng.integers(int(lo), int(hi) + 1))
    inner = np.sort(rng.choice(np.arange(1, bins), size=n - 1, replace=False)) if n > 1 else np.zeros(0, dtype=np.int64)
    edges = np.concatenate([[0], inner, [bins]]).astype(np.int64)
    f = np.arange(bins)
    if s["filter_type"] == "step":
        gains = rng.uniform(-s["filter_db"], s["filter_db"], n)
        return gains[np.searchsorted(edges, f, side="right") - 1]
    gains = rng.uniform(-s["filter_db"], s["filter_db"], n + 1)
    k = np.searchsorted(edges, f, side="right") - 1     # the band of bin f: g_k + (g_k+1 - g_k) (f - e_k) / (e_k+1 - e_k)
    return gains[k] + (gains[k + 1] - gains[k]) * (f - edges[k]) / (edges[k + 1] - edges[k]).astype(np.float64)


def draw_spectral(seed: int, epoch: int, window_indices, cfg, window: int | None = None, bins: int = N_BINS, keys=None):
    """(rows int32 [B, 12], curves float32 [B, 64] or None) of the in-place spectral stage (csrc/spectral.hip, DESIGN.md
    section 26) for the windows ``window_indices`` of ``epoch``: row = [0] frequency shift, [1] flags (bit 0: the window has a
    curve), [2..5] / [6..9] two cutouts (first frame, frames, first bin, bins).  ``curves`` is None when no window has one.

    A window's draw comes from ``np.random.default_rng([seed, epoch, index, 2])`` -- a stream of its own, so ``draw`` and
    ``draw_mix`` ask their generators exactly what they ask without it -- and is a function of (seed, epoch, window index)
    only.  EVERY question is asked, in one fixed order, whatever is switched on, each as one ``random()``: the shift (uniform
    integer in +-AUGMENT_FREQ_SHIFT_MAX), the level (uniform in +-AUGMENT_LEVEL_DB dB), for each of the two cutouts its
    frames (uniform integer in [0, min(AUGMENT_CUTOUT_TIME_MAX, window)]), first frame (uniform over the positions that
    fit), bins and first bin likewise, then u (a filter iff u < AUGMENT_FILTER_PROB) and, only with a filter, its
    variable-length part (``filter_curve``).  So switching one component on never changes another's draw.  The curve of a
    window is level + filter, evaluated in double precision and rounded once; the flag is clear when both are off for it.
    ``keys``: as in ``draw``."""
    s = check_settings(cfg)
    if window is None:
        window = int(int(cfg.WINDOW_LENGTH) / int(cfg.SPECTROGRAM_HOP_LENGTH))
    window = int(window)
    idx = np.asarray(window_indices, dtype=np.int64).reshape(-1)
    rows = identity_spectral_rows(len(idx))
    curves = np.zeros((len(idx), bins), dtype=np.float32)
    if not spectral_enabled(cfg):
        return rows, None
    for r, i in enumerate(_stream_keys(idx, keys)):
        rng = np.random.default_rng([int(seed), int(epoch), int(i), 2])
        rows[r, 0] = _uniform_int(rng.random(), 2 * s["freq_shift_max"] + 1) - s["freq_shift_max"]
        level = (2.0 * rng.random() - 1.0) * s["level_db"]
        for n in range(2):
            u = rng.random(4)
            frames = _uniform_int(u[0], min(s["cutout_time_max"], window) + 1)
            first_frame = _uniform_int(u[1], window - frames + 1)
            width = _uniform_int(u[2], min(s["cutout_freq_max"], bins) + 1)
            first_bin = _uniform_int(u[3], bins - width + 1)
            if n < s["cutouts"]:
                rows[r, 2 + 4 * n:6 + 4 * n] = (first_frame, frames, first_bin, width)
        filtered = rng.random() < s["filter_prob"]
        if filtered or s["level_db"] != 0:
            curve = np.full(bins, level, dtype=np.float64)
            if filtered:
                curve = curve + filter_curve(rng, s, bins)
            rows[r, 1] |= SPECTRAL_CURVE
            curves[r] = curve.astype(np.float32)
    return rows, (curves if (rows[:, 1] & SPECTRAL_CURVE).any() else None)
