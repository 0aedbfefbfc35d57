"""GPU tests of the in-place spectral stage (csrc/spectral.hip, seld_augment.py, dataset.py): the
identity anchor against each of the ten feature exports, the shift, the gain curve, the standardising export and the cutouts
bit for bit against the numpy restatement of tests/spectral_ref.py, one in-place stress batch, the level of a recording
through the dataset path, what the entry points refuse and the training path.  Shapes: 50-frame (and 13-frame) windows on a
150-frame timeline, B = 8 windows of which one runs 40 frames past the end and one starts 20 frames before the timeline."""
import ctypes

import numpy as np
import pytest
import torch
from torch.utils.data import DataLoader

import mic_swap_ref
import mix_ref
import rotate_ref
import spectral_ref
import standardise_ref
from logmel_checks import assert_logmel_close
from oracle import features as ofeat

pytestmark = pytest.mark.gpu

WINDOW, HOP = 50, 10
I, J = 18, 36
TOTAL = 150
STARTS = [0, 10, 30, 57, 90, 100, 140, -20]
CONFIG_NAMES = ("FEATURE_SET", "FOA_CHANNEL_ORDER", "AUGMENT_SPATIAL", "AUGMENT_ROTATE", "AUGMENT_TIME_MASKS",
                "AUGMENT_TIME_MASK_MAX", "AUGMENT_FREQ_MASKS", "AUGMENT_FREQ_MASK_MAX", "AUGMENT_MASK_VALUE", "AUGMENT_MIX_PROB",
                "AUGMENT_MIX_GAIN_DB", "WINDOW_LENGTH", "HOP_LENGTH", "AUGMENT_FREQ_SHIFT_MAX", "AUGMENT_LEVEL_DB",
                "AUGMENT_FILTER_PROB", "AUGMENT_FILTER_DB", "AUGMENT_FILTER_BANDS", "AUGMENT_FILTER_TYPE", "AUGMENT_CUTOUTS",
                "AUGMENT_CUTOUT_TIME_MAX", "AUGMENT_CUTOUT_FREQ_MAX")
INVALID, UNSUPPORTED = -1, -4
# (channels, log-mel channels, mel-axis channels) of 'logmel', 'logmel_iv', 'logmel_nipd' and 'logmel_gcc' of 8 microphones
SETS = {"logmel": (4, 4, 4), "logmel_iv": (7, 4, 7), "logmel_nipd": (15, 8, 15), "logmel_gcc": (36, 8, 8)}


def _bits(a):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else a.dtype)


@pytest.fixture
def class_config():
    """Switches are class attributes (config.py is edited in place upstream; dataset.py and trainer.py each hold an instance)."""
    from config import Config
    saved = {k: getattr(Config, k) for k in CONFIG_NAMES}
    yield Config
    for k, v in saved.items():
        setattr(Config, k, v)


def _timeline(rng, channels, logmel):
    """A feature timeline in the stored formats: the log-mel channels in dB with runs of exact -100 (3 % of the elements and
    two whole frames) and values just above it, the other channels signed around 0."""
    spec = (rng.standard_normal((TOTAL, channels, 64)) * 0.5).astype(np.float32)
    mel = rng.uniform(-99.0, 30.0, (TOTAL, logmel, 64)).astype(np.float32)
    mel[rng.random(mel.shape) < 0.03] = -100.0
    mel[rng.random(mel.shape) < 0.01] = np.float32(-99.99999)
    mel[[5, 62]] = -100.0
    spec[:, :logmel] = mel
    return spec


def _masked_rows(rows, rng, window):
    """Two time and two frequency masks per window in the shapes tests/test_augment_gpu.py cycles through."""
    for r in range(len(rows)):
        kind = r % 4
        if kind == 0:
            tl, fl = rng.integers(0, min(15, window), 2), rng.integers(0, 20, 2)
            rows[r, 1:9] = (rng.integers(0, window - tl[0] + 1), tl[0], rng.integers(0, window - tl[1] + 1), tl[1],
                            rng.integers(0, 64 - fl[0] + 1), fl[0], rng.integers(0, 64 - fl[1] + 1), fl[1])
        elif kind == 1:
            rows[r, 1:9] = (window // 5, 0, window - 1, 0, 0, 0, 63, 0)               # empty
        elif kind == 2:
            rows[r, 1:9] = (0, window // 3, window - 1, 1, 0, 64, 5, 3)               # full width in frequency
        else:
            rows[r, 1:9] = (window - 6, 6, window - 2, 2, 64 - 7, 7, 0, 1)            # touching the ends
    return rows


def _statistics(rng, channels, dev, power_of_two=False):
    if power_of_two:
        scale = (2.0 ** rng.integers(-4, 3, (channels, 64)) * rng.choice([-1.0, 1.0], (channels, 64))).astype(np.float32)
    else:
        scale = (rng.uniform(0.02, 2.0, (channels, 64)) * rng.choice([-1.0, 1.0], (channels, 64))).astype(np.float32)
    shift = (rng.standard_normal((channels, 64)) * 3).astype(np.float32)
    return scale, shift, torch.from_numpy(scale).to(dev), torch.from_numpy(shift).to(dev)


def _staged(dev, x, starts, rows, spectral, curves, logmel, freq, mask_value, scale=None, shift=None, spectral_on_device=False):
    """The stage on the batch x (numpy) with host tables checked and uploaded by seld_native; returns numpy."""
    import seld_native
    B, window = x.shape[:2]
    batch = torch.from_numpy(x.copy()).to(dev)
    params = None if rows is None else seld_native.augment_params(rows, B, window, dev)
    if spectral_on_device:
        spectral_d, curves_d = seld_native.spectral_params(torch.from_numpy(spectral).to(dev),
                                                           None if curves is None else torch.from_numpy(curves).to(dev), B, window, dev)
    else:
        spectral_d, curves_d = seld_native.spectral_params(spectral, curves, B, window, dev)
    got = seld_native.window_spectral(batch, torch.as_tensor(starts), TOTAL, params, spectral_d, curves_d, logmel, freq, mask_value,
                                      scale=scale, shift=shift)
    assert got is batch
    return got.cpu().numpy()


def _gathered(dev, spec, starts, window):
    """The batch as the plain gather writes it (zero rows outside the timeline), as numpy."""
    import seld_native
    return seld_native.gather_windows(torch.from_numpy(spec).to(dev), torch.as_tensor(starts), window).cpu().numpy()


# ------------------------------------------------------------------------------------------ 1. the identity anchor

EXPORTS = ("seld_window_gather", "seld_window_gather_affine", "seld_window_gather_augment", "seld_window_gather_augment_affine",
           "seld_window_gather_rotate", "seld_window_gather_rotate_affine", "seld_window_gather_mix",
           "seld_window_gather_mix_standardised", "seld_window_gather_mic", "seld_window_gather_mic_standardised")


def _gather_of(export, dev, rng, window):
    """(channels, log-mel channels, mel-axis channels, takes rows, call(rows_dev, scale, shift, mask_value, out)) of one
    export on a random timeline."""
    import seld_augment
    import seld_native
    starts = torch.as_tensor(STARTS)
    if "rotate" in export:
        channels, logmel, freq = SETS["logmel_iv"]
        src = torch.from_numpy(_timeline(rng, channels, logmel)).to(dev)
        rot = torch.from_numpy(rng.uniform(0.1, 10.0, (TOTAL, 3, 64)).astype(np.float32)).to(dev)
        table = seld_augment.channel_table("logmel_iv", channels, "WYZX")
        call = lambda rows, scale, shift, mv, out: seld_native.gather_windows_rotate(
            src, rot, starts, window, rows, table, "WYZX", J, freq, mv, out=out, scale=scale, shift=shift)
    elif "mix" in export:
        channels, logmel, freq = SETS["logmel_iv"]
        src = torch.from_numpy(_timeline(rng, channels, logmel)).to(dev)
        table = seld_augment.channel_table("logmel_iv", channels, "WYZX")
        partners = seld_native.mix_partners([50, 0, 100, 0, 77, -20, 120, 10], [3, 0, 9, 12, 0, 5, 1, 0],
                                            [0.5, 0.0, 2.0, 1.0, 0.0, 4.0, 0.25, 1.0], dev)
        call = lambda rows, scale, shift, mv, out: seld_native.gather_windows_mix(
            src, starts, window, rows, partners, table, freq, mv, 3, out=out, scale=scale, shift=shift)
    elif "mic" in export:
        kind = "logmel_gcc" if "standardised" in export else "logmel_nipd"
        channels, logmel, freq = SETS[kind]
        src = torch.from_numpy(_timeline(rng, channels, logmel)).to(dev)
        perm = seld_augment.mic_permutations(mic_swap_ref.cube())
        call = lambda rows, scale, shift, mv, out: seld_native.gather_windows_mic(
            src, starts, window, rows, perm, kind, freq, mv, out=out, scale=scale, shift=shift)
    elif "augment" in export:
        channels, logmel, freq = SETS["logmel"]
        src = torch.from_numpy(_timeline(rng, channels, logmel)).to(dev)
        table = seld_augment.channel_table("logmel", channels, "WYZX")
        call = lambda rows, scale, shift, mv, out: seld_native.gather_windows_augment(
            src, starts, window, rows, table, freq, mv, out=out, scale=scale, shift=shift)
    else:
        channels, logmel, freq = SETS["logmel_gcc"]
        src = torch.from_numpy(_timeline(rng, channels, logmel)).to(dev)
        call = lambda rows, scale, shift, mv, out: (seld_native.gather_windows(src, starts, window, out=out) if scale is None else
                                                    seld_native.gather_windows_affine(src, starts, window, scale, shift, out=out))
    return channels, logmel, freq, export not in ("seld_window_gather", "seld_window_gather_affine"), call


@pytest.mark.parametrize("window", [WINDOW, 13])
@pytest.mark.parametrize("export", EXPORTS)
def test_identity_rows_give_the_gathers_own_masking_and_standardising_export(gpu_device, export, window):
    """The gather called WITHOUT masks and WITHOUT statistics, then the stage with identity spectral rows, the original rows and
    the statistics: bit for bit what the export itself writes with both."""
    import seld_augment
    import seld_native
    dev = gpu_device
    rng = np.random.default_rng(EXPORTS.index(export) * 100 + window)
    channels, logmel, freq, takes_rows, call = _gather_of(export, dev, rng, window)
    with_statistics = "affine" in export or "standardised" in export
    mask_value = -80.0 if EXPORTS.index(export) % 4 < 2 else 0.5
    B = len(STARTS)
    rows = _masked_rows(np.zeros((B, 12), dtype=np.int32), rng, window)
    rows[:, 0] = rng.integers(0, 16, B)
    if "rotate" in export:
        rows[:, 9] = rng.integers(0, J, B)
    if "mic" in export:
        rows[:, 0] = rng.choice(mic_swap_ref.valid_patterns(mic_swap_ref.cube()), B)
    scale = shift = None
    if with_statistics:
        _, _, scale, shift = _statistics(rng, channels, dev)
    params = seld_native.augment_params(rows, B, window, dev, steps=J) if takes_rows else None
    want = call(params, scale, shift, mask_value, None)
    unmasked = rows.copy()
    unmasked[:, 1:9] = 0
    out = torch.full((B, window, channels, 64), float("nan"), device=dev)
    raw = call(seld_native.augment_params(unmasked, B, window, dev, steps=J) if takes_rows else None, None, None, mask_value, out)
    assert raw.data_ptr() == out.data_ptr()
    before = _bits(raw)
    spectral, curves = seld_native.spectral_params(seld_augment.identity_spectral_rows(B), None, B, window, dev)
    got = seld_native.window_spectral(raw, torch.as_tensor(STARTS), TOTAL, params, spectral, curves, logmel, freq, mask_value,
                                      scale=scale, shift=shift)
    assert got.data_ptr() == out.data_ptr()
    assert np.array_equal(_bits(got), _bits(want)), export
    assert not torch.isnan(got).any() and not got[6, 10:].any() and not got[7, :20].any()         # the rows outside stay zero
    if takes_rows:
        assert (want == mask_value).any()
    if with_statistics or takes_rows:                                 # the stage had something to do
        assert not np.array_equal(before, _bits(want))


# ------------------------------------------------------------------------------------------ 2. the shift

SHIFTS = [0, 1, -1, 3, -3, 4, -4, 5, -5, 16, -16, 63, -63]


@pytest.mark.parametrize("feature_set,window", [("logmel", WINDOW), ("logmel_iv", 13), ("logmel_nipd", WINDOW), ("logmel_gcc", WINDOW),
                                                ("logmel_gcc", 13)])
def test_shift_is_an_exact_copy_with_edge_replication(gpu_device, feature_set, window):
    dev = gpu_device
    channels, logmel, freq = SETS[feature_set]
    rng = np.random.default_rng(channels + window)
    shifts = SHIFTS + [1000, -1000]                                   # the last two: a device-resident row, an edge copy
    B = len(shifts)
    starts = [STARTS[n % len(STARTS)] for n in range(B)]
    x = _gathered(dev, _timeline(rng, channels, logmel), starts, window)
    spectral = spectral_ref.rows(shifts)
    got = _staged(dev, x, starts, None, spectral, None, logmel, freq, 0.0, spectral_on_device=True)
    want = spectral_ref.stage(x, starts, TOTAL, None, spectral, None, logmel, freq, 0.0)
    assert np.array_equal(_bits(got), _bits(want))
    assert np.array_equal(_bits(got[0]), _bits(x[0]))                 # s = 0
    assert np.array_equal(_bits(got[:, :, freq:]), _bits(x[:, :, freq:]))            # lag channels: bit-equal to the input
    live = [b for b in range(B) if 0 <= starts[b] and starts[b] + window <= TOTAL]
    for b in live:
        s = max(-64, min(64, shifts[b]))
        for f in (0, 1, 31, 62, 63):
            assert np.array_equal(_bits(got[b, :, :freq, f]), _bits(x[b, :, :freq, min(63, max(0, f - s))])), (b, f)
    for s, edge in ((1000, 0), (-1000, 63)):                          # every bin is the row's edge bin
        b = shifts.index(s)
        assert starts[b] >= 0 and starts[b] < TOTAL and x[b, 0, :freq].any()
        assert np.array_equal(_bits(got[b, :, :freq]), _bits(np.repeat(x[b, :, :freq, edge:edge + 1], 64, axis=-1)))
    # the host check refuses what the device row holds
    import seld_native
    with pytest.raises(ValueError, match="frequency shift"):
        seld_native.spectral_params(spectral, None, B, window, dev)


# ------------------------------------------------------------------------------------------ 3. the gain curve

@pytest.mark.parametrize("feature_set,window", [("logmel", WINDOW), ("logmel_iv", WINDOW), ("logmel_gcc", 13)])
def test_gain_is_one_fp32_addition_above_the_floor(gpu_device, feature_set, window):
    dev = gpu_device
    channels, logmel, freq = SETS[feature_set]
    rng = np.random.default_rng(7 * channels + window)
    B = len(STARTS)
    x = _gathered(dev, _timeline(rng, channels, logmel), STARTS, window)
    curves = rng.uniform(-12.0, 12.0, (B, 64)).astype(np.float32)     # leave values above the floor
    curves[1] = rng.uniform(-150.0, -60.0, 64).astype(np.float32)     # push most values below it
    curves[2, ::2] = -300.0
    curves[4] = 0.0
    flags = [1, 1, 1, 0, 1, 1, 1, 1]                                  # window 3: a curve row that must not be read
    spectral = spectral_ref.rows([0] * B, flags)
    got = _staged(dev, x, STARTS, None, spectral, curves, logmel, freq, 0.0)
    want = spectral_ref.stage(x, STARTS, TOTAL, None, spectral, curves, logmel, freq, 0.0)
    assert np.array_equal(_bits(got), _bits(want))
    assert np.array_equal(_bits(got[3]), _bits(x[3])) and np.array_equal(_bits(got[4]), _bits(x[4]))
    assert np.array_equal(_bits(got[:, :, logmel:]), _bits(x[:, :, logmel:]))        # only the log-mel channels
    floor_in = x[:, :, :logmel] == -100.0
    assert floor_in.sum() > 100 and (got[:, :, :logmel][floor_in] == -100.0).all()   # power 0 stays power 0
    pushed = (got[1, :, :logmel] == -100.0) & (x[1, :, :logmel] > -100.0)
    assert pushed.sum() > 100 and got[:, :, :logmel].min() == -100.0
    # with a shift: the curve is indexed by the destination bin
    spectral[:, 0] = [3, -3, 5, 1, -16, 4, -1, 63]
    got = _staged(dev, x, STARTS, None, spectral, curves, logmel, freq, 0.0)
    want = spectral_ref.stage(x, STARTS, TOTAL, None, spectral, curves, logmel, freq, 0.0)
    assert np.array_equal(_bits(got), _bits(want))
    # curves = None: no window has one, whatever the flags say
    got = _staged(dev, x, STARTS, None, spectral_ref.rows([0] * B, flags), None, logmel, freq, 0.0)
    assert np.array_equal(_bits(got), _bits(x))


# ------------------------------------------------------------------------------------------ 4. the standardising export

@pytest.mark.parametrize("feature_set", ["logmel_iv", "logmel_gcc"])
def test_standardised_export_against_the_restatement(gpu_device, feature_set):
    dev = gpu_device
    channels, logmel, freq = SETS[feature_set]
    rng = np.random.default_rng(11 * channels)
    B = len(STARTS)
    x = _gathered(dev, _timeline(rng, channels, logmel), STARTS, WINDOW)
    rows = _masked_rows(np.zeros((B, 12), dtype=np.int32), rng, WINDOW)
    curves = rng.uniform(-12.0, 12.0, (B, 64)).astype(np.float32)
    cuts = [((3, 10, 5, 20), (40, 10, 60, 4))] * B
    spectral = spectral_ref.rows([2, -5, 0, 7, -1, 4, 3, -16], [1, 0, 1, 1, 0, 1, 1, 1], cuts)
    # power-of-two scales: the product is exact, so the restatement's v * scale + shift rounds once as the fused multiply-add
    scale, shift, scale_d, shift_d = _statistics(rng, channels, dev, power_of_two=True)
    got = _staged(dev, x, STARTS, rows, spectral, curves, logmel, freq, -80.0, scale_d, shift_d)
    want = spectral_ref.stage(x, STARTS, TOTAL, rows, spectral, curves, logmel, freq, -80.0, scale, shift)
    assert np.array_equal(_bits(got), _bits(want))
    unmapped = spectral_ref.stage(x, STARTS, TOTAL, None, spectral_ref.rows(spectral[:, 0], spectral[:, 1]), curves, logmel, freq, 0.0)
    assert np.array_equal(_bits(want[1, 20, 2]), _bits(standardise_ref.affine_exact_scale(unmapped[1, 20, 2], scale[2], shift[2])))
    # real statistics: within one fp32 ulp of the float64 evaluation of the map on the fp32 value in front of it
    scale, shift, scale_d, shift_d = _statistics(rng, channels, dev)
    got = _staged(dev, x, STARTS, rows, spectral, curves, logmel, freq, -80.0, scale_d, shift_d)
    front = spectral_ref.stage(x, STARTS, TOTAL, None, spectral_ref.rows(spectral[:, 0], spectral[:, 1]), curves, logmel, freq, 0.0)
    want64 = spectral_ref.stage(front, STARTS, TOTAL, rows, spectral_ref.rows([0] * B, None, cuts), None, logmel, freq, -80.0,
                                scale, shift, dtype=np.float64)
    err = np.abs(got.astype(np.float64) - want64) / standardise_ref.ulp32(want64)
    print(f"{feature_set}: worst error {err.max():.3f} ulp")
    assert err.max() <= 1.0
    masked = want64 == -80.0
    assert masked.any() and (got[masked] == np.float32(-80.0)).all() and not got[6, 10:].any() and not got[7, :20].any()


# ------------------------------------------------------------------------------------------ 5. the cutouts

@pytest.mark.parametrize("feature_set,window", [("logmel_iv", WINDOW), ("logmel_gcc", WINDOW), ("logmel_gcc", 13)])
def test_cutouts_blank_rectangles_on_the_mel_axis_channels(gpu_device, feature_set, window):
    dev = gpu_device
    channels, logmel, freq = SETS[feature_set]
    rng = np.random.default_rng(13 * channels + window)
    B = len(STARTS)
    x = _gathered(dev, _timeline(rng, channels, logmel), STARTS, window)
    w = window
    cuts = [((0, 0, 0, 0), (5, 0, 10, 8)),                           # empty
            ((0, w, 0, 64), (0, 0, 0, 0)),                           # the whole window
            ((0, 3, 0, 5), (w - 2, 2, 60, 4)),                       # touching the edges
            ((2, 8, 10, 20), (6, 6, 25, 20)),                        # overlapping each other
            ((4, 5, 0, 64), (0, w, 30, 2)),                          # overlapping the masks of this window's row
            ((3, 4, 7, 0), (9, 1, 63, 1)),                           # zero width; a single element
            ((0, w, 3, 9), (w - 1, 1, 0, 64)),                       # on the tail window (starts 140: frames 10.. are outside)
            ((0, w, 50, 14), (w // 2, w - w // 2, 0, 6))]            # on the window that begins before the timeline
    rows = np.zeros((B, 12), dtype=np.int32)
    rows[4, 1:9] = (5, 3, 0, 0, 28, 6, 0, 0)
    spectral = spectral_ref.rows([0] * B, None, cuts)
    for mask_value in (0.0, -80.0):
        got = _staged(dev, x, STARTS, rows, spectral, None, logmel, freq, mask_value)
        want = spectral_ref.stage(x, STARTS, TOTAL, rows, spectral, None, logmel, freq, mask_value)
        assert np.array_equal(_bits(got), _bits(want))
        assert np.array_equal(_bits(got[0]), _bits(x[0]))
        assert (got[1, :, :freq] == np.float32(mask_value)).all()
        keep = np.ones(got.shape, dtype=bool)
        keep[4, 5:8] = False                                          # the time mask of window 4 covers every channel
        assert np.array_equal(_bits(got[:, :, freq:][keep[:, :, freq:]]), _bits(x[:, :, freq:][keep[:, :, freq:]]))
        assert not got[6, 10:].any() and not got[7, :min(20, w)].any()               # rows outside: never the mask value
    assert (want == np.float32(-80.0)).sum() > 64 * w


# ------------------------------------------------------------------------------------------ 6. in place, many windows

def test_in_place_on_a_large_batch_with_everything_drawn(gpu_device):
    """B = 64 windows of 36 channels, every window with a random shift, curve, cutouts and masks: 115 200 rows whose lanes
    exchange bins while their neighbours store.  One run, element for element against the restatement."""
    dev = gpu_device
    channels, logmel, freq = SETS["logmel_gcc"]
    rng = np.random.default_rng(2026)
    B = 64
    starts = [int(s) for s in rng.integers(-30, TOTAL - 10, B)]
    x = _gathered(dev, _timeline(rng, channels, logmel), starts, WINDOW)
    rows = _masked_rows(np.zeros((B, 12), dtype=np.int32), rng, WINDOW)
    shifts = rng.integers(-63, 64, B)
    cuts = []
    for _ in range(B):
        tl, fl = rng.integers(0, 30, 2), rng.integers(0, 20, 2)
        cuts.append(tuple((int(rng.integers(0, WINDOW - tl[n] + 1)), int(tl[n]), int(rng.integers(0, 64 - fl[n] + 1)), int(fl[n]))
                          for n in range(2)))
    spectral = spectral_ref.rows(shifts, rng.integers(0, 2, B), cuts)
    curves = rng.uniform(-12.0, 12.0, (B, 64)).astype(np.float32)
    got = _staged(dev, x, starts, rows, spectral, curves, logmel, freq, -80.0)
    want = spectral_ref.stage(x, starts, TOTAL, rows, spectral, curves, logmel, freq, -80.0)
    assert got.shape == (64, 50, 36, 64) and np.array_equal(_bits(got), _bits(want))
    assert not np.array_equal(_bits(got), _bits(x)) and set(np.unique(shifts % 4)) == {0, 1, 2, 3}
    # a window with nothing drawn among the others is not rewritten: what was there stays, bit for bit
    spectral[::3] = 0
    rows[::3] = 0
    got = _staged(dev, x, starts, rows, spectral, curves, logmel, freq, -80.0)
    assert np.array_equal(_bits(got[::3]), _bits(x[::3]))
    assert np.array_equal(_bits(got), _bits(spectral_ref.stage(x, starts, TOTAL, rows, spectral, curves, logmel, freq, -80.0)))


# ------------------------------------------------------------------------------------------ 7. the level, on the device

def _dataset(Config, dev, feature_set, order, clips, rows, window=WINDOW, hop=HOP):
    import dataset
    Config.FEATURE_SET, Config.FOA_CHANNEL_ORDER, Config.AUGMENT_ROTATE = feature_set, order, False
    Config.WINDOW_LENGTH, Config.HOP_LENGTH = window * 480, hop * 480
    return dataset.SELDDataset.from_pcm(clips, rows, device=dev)


def test_a_constant_curve_is_the_level_of_the_recording(gpu_device, class_config):
    """Features of the clips scaled by a = 0.5 and 2 through the dataset path against the stage with the constant curve
    20 log10 a on the unscaled clips' features: 2e-4 dB over the elements within 40 dB of their frame's peak, each side being
    within 1e-4 dB of the float64 oracle there (tests/logmel_checks.py).  Measured maximum: see DESIGN.md section 26.4."""
    dev = gpu_device
    clips = [rotate_ref.plane_wave_clip("WYZX", n) for n in range(3)]
    meta = [rotate_ref.clip_rows() for _ in clips]
    ds = _dataset(class_config, dev, "logmel_iv", "WYZX", clips, meta)
    idx = [0, 5, 10]                                                  # starts 0, 50, 100: the three clips
    assert ds.total_frames == TOTAL and np.array_equal(ds.window_starts[idx], [0, 50, 100])
    plain = ds.device_batch(idx)[0].cpu().numpy()
    worst = 0.0
    for a in (0.5, 2.0):
        scaled = [(a * c.double()).float() for c in clips]
        ds_a = _dataset(class_config, dev, "logmel_iv", "WYZX", scaled, meta)
        side_a = ds_a.device_batch(idx)[0].cpu().numpy()              # [3, 50, 7, 64]
        curve = np.full((3, 64), 20.0 * np.log10(a), dtype=np.float32)
        side_b = ds.device_batch(idx, spectral=(spectral_ref.rows([0, 0, 0], [1, 1, 1]), curve))[0].cpu().numpy()
        oracle = np.stack([ofeat.logmel_f64(c.numpy().astype(np.float64))[:, :, :50].transpose(2, 0, 1) for c in scaled])
        assert_logmel_close(side_a[:, :, :4], oracle, mel_axis=-1)
        strong = oracle >= oracle.max(axis=-1, keepdims=True) - 40.0
        assert np.abs(side_b[:, :, :4].astype(np.float64) - oracle)[strong].max() <= 1e-4
        err = np.abs(side_a[:, :, :4].astype(np.float64) - side_b[:, :, :4])[strong].max()
        worst = max(worst, float(err))
        print(f"a = {a}: max |dB difference| over {int(strong.sum())} of {strong.size} elements {err:.3e}")
        assert err <= 2e-4
        assert np.array_equal(_bits(side_b[:, :, 4:]), _bits(plain[:, :, 4:]))       # the intensity channels: untouched
        assert not np.array_equal(_bits(side_b[:, :, :4]), _bits(plain[:, :, :4]))
    print(f"level on the device: worst {worst:.3e} dB")


# ------------------------------------------------------------------------------------------ 8. entry refusals

NAMES = ("seld_window_spectral", "seld_window_spectral_standardised")


def _cases():
    rows = []
    for name in NAMES:
        pointers = ("batch", "starts", "params", "spectral", "curves", "scale", "shift")
        rows += [(name, "total_rows = -1", {"total_rows": -1}, INVALID), (name, "B = -1", {"B": -1}, INVALID),
                 (name, "window = 0", {"window": 0}, INVALID), (name, "window = -3", {"window": -3}, INVALID),
                 (name, "channels = 0", {"channels": 0, "logmel": 0, "freq": 0}, INVALID),
                 (name, "channels = -1", {"channels": -1, "logmel": 0, "freq": 0}, INVALID),
                 (name, "logmel_channels = -1", {"logmel": -1}, INVALID),
                 (name, "logmel_channels > freq_channels", {"logmel": 4, "freq": 3}, INVALID),
                 (name, "freq_channels > channels", {"freq": 5}, INVALID),
                 (name, "2^31 chunks in a window", {"window": (1 << 31) // 64}, UNSUPPORTED),
                 (name, "B = 0, 2^31 chunks in a window", {"B": 0, "window": (1 << 31) // 64}, UNSUPPORTED),
                 (name, "B = 0, freq_channels > channels", {"B": 0, "freq": 5}, INVALID),
                 (name, "B = 1, null batch", {"batch": None}, INVALID), (name, "B = 1, null starts", {"starts": None}, INVALID),
                 (name, "B = 1, null spectral", {"spectral": None}, INVALID),
                 (name, "B = 0, every pointer null", dict({p: None for p in pointers}, B=0), 0)]
    rows += [(NAMES[1], "B = 1, null scale", {"scale": None}, INVALID), (NAMES[1], "B = 1, null shift", {"shift": None}, INVALID)]
    return rows


CASES = _cases()


@pytest.fixture(scope="module")
def library(gpu_device):
    import seld_native
    seld_native.ensure_init(gpu_device)
    buf = torch.full((1024,), 77.0, dtype=torch.float32, device=gpu_device)
    assert buf.data_ptr() % 16 == 0
    yield seld_native.load_library(), buf, seld_native._stream_ptr(gpu_device)
    torch.cuda.synchronize(gpu_device)
    assert bool((buf == 77.0).all())                                           # nothing was launched on it


@pytest.mark.parametrize("name,case,overrides,expected", CASES, ids=[f"{c[0]}-{c[1]}" for c in CASES])
def test_entry_point_refuses(library, name, case, overrides, expected):
    """Every case is refused before the launch (or is an empty call), so nothing runs on the device."""
    lib, buf, stream = library
    p = ctypes.c_void_p(buf.data_ptr())
    a = {"batch": p, "starts": p, "params": p, "spectral": p, "curves": p, "scale": p, "shift": p, "total_rows": 1, "B": 1,
         "window": 1, "channels": 4, "logmel": 4, "freq": 4}
    a.update(overrides)
    head = (a["batch"], a["total_rows"], a["channels"], a["logmel"], a["freq"], a["starts"], a["params"], a["spectral"], a["curves"],
            a["B"], a["window"], 0.0)
    if name == NAMES[0]:
        rc = lib.seld_window_spectral(*head, stream)
    else:
        rc = lib.seld_window_spectral_standardised(*head, a["scale"], a["shift"], stream)
    print(name, case, rc, lib.seld_last_error())
    assert rc == expected
    if expected:
        assert lib.seld_last_error().startswith(name.encode() + b":")


def test_bindings_refuse_tensors_of_the_wrong_kind(gpu_device):
    import seld_native
    dev = gpu_device
    batch = torch.zeros((2, WINDOW, 4, 64), device=dev)
    starts = torch.zeros(2, dtype=torch.int64)
    spectral = torch.zeros((2, 12), dtype=torch.int32, device=dev)
    for bad in (torch.zeros((2, 12), dtype=torch.int32), torch.zeros((2, 12), dtype=torch.int64, device=dev),
                torch.zeros((3, 12), dtype=torch.int32, device=dev), None):
        with pytest.raises(ValueError, match="spectral"):
            seld_native.window_spectral(batch, starts, TOTAL, None, bad, None, 4, 4)
    with pytest.raises(ValueError, match="curves"):
        seld_native.window_spectral(batch, starts, TOTAL, None, spectral, torch.zeros((2, 64)), 4, 4)
    with pytest.raises(ValueError, match="params"):
        seld_native.window_spectral(batch, starts, TOTAL, torch.zeros((2, 12), device=dev), spectral, None, 4, 4)
    with pytest.raises(ValueError, match="come together"):
        seld_native.window_spectral(batch, starts, TOTAL, None, spectral, None, 4, 4, scale=torch.ones((4, 64), device=dev))
    with pytest.raises(seld_native.SeldNativeError, match="batch"):
        seld_native.window_spectral(batch[:, :, :, :32], starts, TOTAL, None, spectral, None, 4, 4)
    with pytest.raises(seld_native.SeldNativeError, match="-1"):
        seld_native.window_spectral(batch, starts, TOTAL, None, spectral, None, 5, 4)
    assert seld_native.window_spectral(batch, starts, TOTAL, None, spectral, None, 4, 4) is batch


# ------------------------------------------------------------------------------------------ 9. the dataset and training path

def test_device_batch_takes_every_branch_of_the_dispatch(gpu_device, class_config):
    """plain, augmenting, mixing, rotating and array datasets, with and without statistics: identity spectral rows give the
    batch ``device_batch`` returns without ``spectral``, bit for bit, labels included; drawn rows change the features only."""
    import dataset
    import seld_augment
    dev = gpu_device
    clips = [rotate_ref.plane_wave_clip("WYZX", n) for n in range(3)]
    meta = [rotate_ref.clip_rows() for _ in clips]
    idx = [0, 4, 14, 9]
    rng = np.random.default_rng(5)
    rows = _masked_rows(np.zeros((4, 12), dtype=np.int32), rng, WINDOW)
    rows[:, 0] = [3, 0, 9, 12]
    mix = (np.asarray([3, -1, 0, 7]), np.asarray([5, 0, 0, 2], np.int32), np.asarray([1.0, 0.0, 2.0, 0.5], np.float32))
    identity = (seld_augment.identity_spectral_rows(4), None)
    drawn = (spectral_ref.rows([3, -2, 0, 5], [1, 0, 1, 0], [((2, 9, 4, 11), (0, 0, 0, 0))] * 4),
             np.full((4, 64), -3.0, dtype=np.float32))
    ds = _dataset(class_config, dev, "logmel_iv", "WYZX", clips, meta)
    class_config.AUGMENT_ROTATE = True
    with_terms = dataset.SELDDataset.from_pcm(clips, meta, device=dev)
    class_config.AUGMENT_ROTATE = False
    turned = rows.copy()
    turned[:, 0] &= 9
    turned[:, 9] = [5, 0, 17, 35]
    cases = [(ds, {}), (ds, {"augment": rows}), (ds, {"augment": rows, "mix": mix}), (with_terms, {"augment": turned})]
    for statistics in (False, True):
        if statistics:
            scale, shift = (torch.from_numpy(t) for t in _statistics(rng, 7, dev)[:2])
            for d in (ds, with_terms):
                d.set_feature_statistics({"scale": scale, "shift": shift, "mean": torch.zeros(7, 64)})
        for d, kw in cases:
            want_s, want_m = d.device_batch(idx, **kw)
            got_s, got_m = d.device_batch(idx, spectral=identity, **kw)
            assert np.array_equal(_bits(got_s), _bits(want_s)) and np.array_equal(_bits(got_m), _bits(want_m)), (statistics, list(kw))
            new_s, new_m = d.device_batch(idx, spectral=drawn, **kw)
            assert np.array_equal(_bits(new_m), _bits(want_m)) and not np.array_equal(_bits(new_s), _bits(want_s))
            assert np.array_equal(_bits(new_s[2, 10:]), _bits(want_s[2, 10:])) and not new_s[2, 10:].any()    # the tail's zero rows
    with pytest.raises(ValueError, match="frequency shift"):
        ds.device_batch(idx, spectral=(spectral_ref.rows([64, 0, 0, 0]), None))
    with pytest.raises(ValueError, match="spectral"):
        ds.device_batch(idx, spectral=identity[0])


@pytest.mark.parametrize("mix_prob", [0.0, 0.5])
def test_training_with_the_stage_is_reproducible_and_evaluation_is_untouched(gpu_device, class_config, tmp_path, mix_prob):
    """train_model runs (small CRNN, captured steps, SEED set) with every new switch on, AUGMENT_SPATIAL and masks give
    identical loss histories, which differ from the run with the new switches off; a window's batch differs between epoch 1
    and epoch 2; the evaluation feed of the same process returns un-augmented windows; with the defaults the stage is never
    called.  mix_prob = 0.5: the shorter case on the mixing pair."""
    import seld_native
    import trainer
    cfg = trainer.config
    names = ("MODEL_TYPE", "CRNN_CNN_CHANNELS", "CRNN_RNN_HIDDEN", "CRNN_DROPOUT", "NUM_EPOCHS", "BATCH_SIZE", "SEED",
             "OUTPUT_PATH", "CHECKPOINT_PATH", "GRAPH_STEP", "DEVICE_FEED")
    saved = {k: getattr(cfg, k) for k in names}
    saved_det = torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark
    shadowed = "FEATURE_SET" in vars(cfg)                 # an earlier test may have left an instance attribute over the class's
    shadow = vars(cfg).get("FEATURE_SET")
    calls = []
    real = seld_native.window_spectral

    def counted(*a, **k):
        calls.append(1)
        return real(*a, **k)

    on = dict(AUGMENT_FREQ_SHIFT_MAX=4, AUGMENT_LEVEL_DB=6.0, AUGMENT_FILTER_PROB=0.5, AUGMENT_CUTOUTS=2, AUGMENT_CUTOUT_TIME_MAX=40,
              AUGMENT_CUTOUT_FREQ_MAX=12)
    off = dict(AUGMENT_FREQ_SHIFT_MAX=0, AUGMENT_LEVEL_DB=0.0, AUGMENT_FILTER_PROB=0.0, AUGMENT_CUTOUTS=0, AUGMENT_CUTOUT_TIME_MAX=0,
               AUGMENT_CUTOUT_FREQ_MAX=0)
    try:
        seld_native.window_spectral = counted
        cfg.FEATURE_SET = "logmel_iv"
        torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = True, False
        cfg.MODEL_TYPE, cfg.CRNN_CNN_CHANNELS, cfg.CRNN_RNN_HIDDEN, cfg.CRNN_DROPOUT = "crnn", [8, 8, 16, 16], 16, 0.0
        cfg.NUM_EPOCHS, cfg.BATCH_SIZE, cfg.SEED, cfg.GRAPH_STEP, cfg.DEVICE_FEED = (1 if mix_prob else 2), 4, 11, True, True
        cfg.OUTPUT_PATH, cfg.CHECKPOINT_PATH = tmp_path / "outputs", tmp_path / "checkpoints"
        cfg.OUTPUT_PATH.mkdir()
        cfg.CHECKPOINT_PATH.mkdir()
        clips = [rotate_ref.plane_wave_clip("WYZX", n) for n in range(18)]
        rows = [mix_ref.clip_rows(n % 4) for n in range(18)]
        train_ds = _dataset(class_config, gpu_device, "logmel_iv", "WYZX", clips[:12], rows[:12], window=250, hop=50)
        test_ds = _dataset(class_config, gpu_device, "logmel_iv", "WYZX", clips[12:], rows[12:], window=250, hop=50)
        train_loader = DataLoader(train_ds, batch_size=cfg.BATCH_SIZE, shuffle=True)
        test_loader = DataLoader(test_ds, batch_size=cfg.BATCH_SIZE, shuffle=False)
        class_config.AUGMENT_SPATIAL, class_config.AUGMENT_MIX_PROB = True, mix_prob
        class_config.AUGMENT_TIME_MASKS, class_config.AUGMENT_TIME_MASK_MAX = 1, 30
        class_config.AUGMENT_FREQ_MASKS, class_config.AUGMENT_FREQ_MASK_MAX = 1, 8

        def run(switches):
            for k, v in switches.items():
                setattr(class_config, k, v)
            assert trainer.graph_step_enabled(gpu_device, 1)
            for old in cfg.CHECKPOINT_PATH.glob("*.pth"):
                old.unlink()
            calls.clear()
            _, history = trainer.train_model(train_loader=train_loader, test_loader=test_loader, device=gpu_device)
            assert history["total_epochs"] == cfg.NUM_EPOCHS and history["config"]["batch_source"] == "DeviceFeed"
            return (history["train_losses"], history["test_losses"]), len(calls)

        (first, n_first), (second, _) = run(on), run(on)
        print("stage on:", first, "again:", second, "calls:", n_first)
        assert np.isfinite(first[0]).all() and np.isfinite(first[1]).all() and first == second
        assert n_first == cfg.NUM_EPOCHS * 3                          # 12 windows in batches of 4: once per training batch only
        if mix_prob:
            return
        base, n_base = run(off)
        print("stage off:", base)
        assert n_base == 0 and first[0] != base[0]

        for k, v in on.items():
            setattr(class_config, k, v)
        n = len(train_ds)
        feed = trainer.make_feed(DataLoader(train_ds, batch_size=n, shuffle=False), gpu_device, 0, 1)
        e1 = [t.clone() for t in next(iter(feed.batches(1, augment=True)))]
        e1_again = [t.clone() for t in next(iter(feed.batches(1, augment=True)))]
        e2 = [t.clone() for t in next(iter(feed.batches(2, augment=True)))]
        assert torch.equal(e1[0].view(torch.int32), e1_again[0].view(torch.int32)) and torch.equal(e1[1], e1_again[1])
        for w in range(n):
            assert not torch.equal(e1[0][w], e2[0][w]), w
        plain = train_ds.device_batch(list(range(n)))
        calls.clear()
        for got in (next(iter(feed.batches(1))), next(iter(feed.batches(0, augment=False)))):
            assert torch.equal(got[0].view(torch.int32), plain[0].view(torch.int32))
            assert torch.equal(got[1].view(torch.int16), plain[1].view(torch.int16))
        results_on = trainer.test_model(test_loader=test_loader, model_path=cfg.CHECKPOINT_PATH / "best_model.pth",
                                        device=gpu_device, num_visualizations=1, save_visualizations=False)
        for k, v in off.items():
            setattr(class_config, k, v)
        results_off = trainer.test_model(test_loader=test_loader, model_path=cfg.CHECKPOINT_PATH / "best_model.pth",
                                         device=gpu_device, num_visualizations=1, save_visualizations=False)
        assert results_on["test_loss"] == results_off["test_loss"] and not calls
    finally:
        seld_native.window_spectral = real
        torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = saved_det
        for k, v in saved.items():
            setattr(cfg, k, v)
        if shadowed:
            cfg.FEATURE_SET = shadow
        else:
            del cfg.FEATURE_SET
