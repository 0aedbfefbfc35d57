"""GPU tests of the two-window mix of the device gather (csrc/mix.hip, seld_augment.py): the copy path
bit-equal to the augmenting pair, the mixed path against the float64 restatement of tests/mix_ref.py, the united labels, what
the entry points refuse, the physics (the mixed recording built from scratch) and the training path.  Shapes: 50-frame
windows with hop 10 on a 150-frame timeline, B = 8 windows of which the last runs 40 frames past the end."""
import ctypes

import numpy as np
import pytest
import torch
from torch.utils.data import DataLoader

import mix_ref
import rotate_ref
from oracle import features as ofeat

pytestmark = pytest.mark.gpu

WINDOW, HOP = 50, 10
I, J = 18, 36
TOTAL = 150
STARTS = [0, 10, 30, 57, 90, 100, 120, 140]
CONFIG_NAMES = ("FEATURE_SET", "FOA_CHANNEL_ORDER", "AUGMENT_SPATIAL", "AUGMENT_ROTATE", "AUGMENT_TIME_MASKS",
                "AUGMENT_TIME_MASK_MAX", "AUGMENT_FREQ_MASKS", "AUGMENT_FREQ_MASK_MAX", "AUGMENT_MASK_VALUE", "AUGMENT_MIX_PROB",
                "AUGMENT_MIX_GAIN_DB", "WINDOW_LENGTH", "HOP_LENGTH")
INVALID, UNSUPPORTED = -1, -4


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else a.dtype)


@pytest.fixture
def class_config():
    """Switches are class attributes (config.py is edited in place upstream; dataset.py and trainer.py each hold an instance)."""
    from config import Config
    saved = {k: getattr(Config, k) for k in CONFIG_NAMES}
    yield Config
    for k, v in saved.items():
        setattr(Config, k, v)


def _dataset(Config, dev, feature_set, order, clips, rows, window=WINDOW, hop=HOP):
    import dataset
    Config.FEATURE_SET, Config.FOA_CHANNEL_ORDER, Config.AUGMENT_ROTATE = feature_set, order, False
    Config.WINDOW_LENGTH, Config.HOP_LENGTH = window * 480, hop * 480
    return dataset.SELDDataset.from_pcm(clips, rows, device=dev)


def _masked_rows(rows, rng, window=WINDOW):
    """Time / frequency masks in the shapes tests/test_augment_gpu.py cycles through, on top of the patterns given."""
    for r in range(len(rows)):
        kind = r % 4
        if kind == 0:
            tl, fl = rng.integers(0, 15, 2), rng.integers(0, 20, 2)
            rows[r, 1:9] = (rng.integers(0, window - tl[0] + 1), tl[0], rng.integers(0, window - tl[1] + 1), tl[1],
                            rng.integers(0, 64 - fl[0] + 1), fl[0], rng.integers(0, 64 - fl[1] + 1), fl[1])
        elif kind == 1:
            rows[r, 1:9] = (10, 0, window - 1, 0, 0, 0, 63, 0)                       # empty
        elif kind == 2:
            rows[r, 1:9] = (0, 20, window - 1, 1, 0, 64, 5, 3)                       # full width in frequency
        else:
            rows[r, 1:9] = (window - 6, 6, window - 2, 2, 64 - 7, 7, 0, 1)          # touching the ends
    return rows


def _timeline(rng, channels, iv_channels):
    """A feature timeline in the stored formats: log-mel channels in dB over the whole range the floor rule sees (-100
    exactly on 3 % of the elements and on two whole frames, values just above it, up to +30 dB), intensity channels signed."""
    spec = rng.uniform(-99.0, 30.0, (TOTAL, channels, 64)).astype(np.float32)
    spec[rng.random(spec.shape) < 0.03] = -100.0
    spec[rng.random(spec.shape) < 0.01] = np.float32(-99.99999)
    spec[[5, 62]] = -100.0                                           # silence: frames 5 and 62 of every channel
    if iv_channels:
        iv = (rng.standard_normal((TOTAL, iv_channels, 64)) * 0.5).astype(np.float32)
        iv[rng.random(iv.shape) < 0.01] = 0.0
        iv[rng.random(iv.shape) < 0.01] = -0.0
        spec[:, channels - iv_channels:] = iv
    mask = np.where(rng.random((TOTAL, I * J)) < 0.03, rng.integers(1, 1 << 13, (TOTAL, I * J)), 0).astype(np.uint16)
    return spec, mask


def _affine(rng, channels, dev):
    scale = (rng.uniform(0.5, 2.0, (channels, 64)) * rng.choice([-1.0, 1.0], (channels, 64))).astype(np.float32)
    shift = rng.standard_normal((channels, 64)).astype(np.float32)
    return scale, shift, torch.from_numpy(scale).to(dev), torch.from_numpy(shift).to(dev)


def _table(channels, order):
    import seld_augment
    return seld_augment.channel_table("logmel_iv" if channels == 7 else "logmel", channels, order or "WYZX")


# ------------------------------------------------------------------------------------------ 1. the copy path

@pytest.mark.parametrize("channels,order,mask_value,with_out,affine", [(4, "WYZX", 0.0, False, False), (4, "WXYZ", -80.0, True, True),
                                                                      (7, "WYZX", -80.0, True, False), (7, "WXYZ", 0.0, False, True)])
def test_frames_without_a_partner_row_are_bit_equal_to_the_augmenting_pair(gpu_device, channels, order, mask_value, with_out,
                                                                            affine):
    """No partner = a gain of 0, -0, NaN, negative or infinite, with garbage in the other fields of the row; or a partner
    whose frame lies outside the timeline (sb negative, past the end, +-2^62).  Those frames are what
    seld_window_gather_augment(_affine) / seld_window_permute_mask write, bit for bit -- masks, zero rows and all."""
    import seld_native
    dev = gpu_device
    rng = np.random.default_rng(channels + affine)
    iv = 3 if channels == 7 else 0
    spec, mask = _timeline(rng, channels, iv)
    table = _table(channels, order)
    assert np.array_equal(table, mix_ref.channel_table(channels, order))
    no_gain = [0.0, -0.0, float("nan"), -1.0, float("inf"), -float("inf"), -1e-30, -float("nan")]
    outside = [-WINDOW, -10000, TOTAL, TOTAL + 7, 1 << 62, -(1 << 62), (1 << 63) - 60, -(1 << 63)]
    partial = [(-20, range(0, 20)), (120, range(30, WINDOW)), (-49, range(0, 49)), (149, range(1, WINDOW))]   # (sb, the copy frames)
    B = len(no_gain) + len(outside) + len(partial)
    rows = _masked_rows(np.zeros((B, 12), dtype=np.int32), rng)
    rows[B - len(partial):, 1:9] = 0                                  # the partial windows: one small mask, so mixed frames show
    rows[B - len(partial), 1:9] = (5, 3, 0, 0, 10, 4, 0, 0)
    rows[:, 0] = rng.integers(0, 16, B)
    starts = [(STARTS + [TOTAL, -20])[n % 10] for n in range(B)]
    for n in range(len(partial)):
        starts[len(no_gain) + len(outside) + n] = (0, 10, 57, 100)[n]               # live windows for the partial partners
    words = np.zeros((B, 2), dtype=np.uint64)
    garbage = rng.integers(0, 1 << 63, B, dtype=np.uint64) << np.uint64(1)
    for n in range(B):
        if n < len(no_gain):
            sb, g = int(rng.integers(0, TOTAL - WINDOW)), no_gain[n]                 # an in-range start: it would mix if it could
        elif n < len(no_gain) + len(outside):
            sb, g = outside[n - len(no_gain)], 2.0
        else:
            sb, g = partial[n - len(no_gain) - len(outside)][0], 0.5
        words[n, 0] = np.uint64(sb & 0xFFFFFFFFFFFFFFFF)
        words[n, 1] = (garbage[n] & np.uint64(0xFFFFFFFF00000000)) | np.uint64(int(np.float32(g).view(np.uint32)))
    partners_host = words.view(np.int64)
    for n in range(len(no_gain)):
        assert not mix_ref.unpack_partner(partners_host[n])[3]
    partners = torch.from_numpy(partners_host.copy()).to(dev)
    spec_d, mask_d = torch.from_numpy(spec).to(dev), torch.from_numpy(mask).to(dev)
    scale = shift = None
    if affine:
        _, _, scale, shift = _affine(rng, channels, dev)
    params = seld_native.augment_params(rows, B, WINDOW, dev)
    starts_t = torch.as_tensor(starts)
    out_s = torch.full((B, WINDOW, channels, 64), float("nan"), device=dev) if with_out else None
    out_m = torch.from_numpy(np.full((B, WINDOW, I * J), 0xFFFF, dtype=np.uint16)).to(dev) if with_out else None
    got_s = seld_native.gather_windows_mix(spec_d, starts_t, WINDOW, params, partners, table, channels, mask_value, iv, out=out_s,
                                           scale=scale, shift=shift)
    got_m = seld_native.gather_windows_mix_mask(mask_d, starts_t, WINDOW, params, partners, I, J, out=out_m)
    if with_out:
        assert got_s.data_ptr() == out_s.data_ptr() and got_m.data_ptr() == out_m.data_ptr()
    want_s = seld_native.gather_windows_augment(spec_d, starts_t, WINDOW, params, table, channels, mask_value, scale=scale, shift=shift)
    want_m = seld_native.gather_windows_permute(mask_d, starts_t, WINDOW, params, I, J)
    whole = B - len(partial)
    assert torch.equal(got_s[:whole].view(torch.int32), want_s[:whole].view(torch.int32))
    assert torch.equal(got_m[:whole].view(torch.int16), want_m[:whole].view(torch.int16))
    for n, (_, frames) in enumerate(partial):
        b, frames = whole + n, list(frames)
        mixed = [w for w in range(WINDOW) if w not in frames]
        assert torch.equal(got_s[b, frames].view(torch.int32), want_s[b, frames].view(torch.int32)), n
        assert torch.equal(got_m.view(torch.int16)[b, frames], want_m.view(torch.int16)[b, frames]), n
        assert not torch.equal(got_s[b, mixed].view(torch.int32), want_s[b, mixed].view(torch.int32)), n
    assert (want_s == mask_value).any() and want_m.cpu().numpy().any() and not torch.isnan(got_s).any()


# ------------------------------------------------------------------------------------------ 2. the mixed path vs float64

PAIRS = [(0, 0), (8, 0), (0, 8), (2, 0), (0, 2), (4, 0), (0, 4), (1, 0), (0, 1), (2, 9), (15, 6), (9, 13), (6, 6), (3, 12), (0, 0),
         (5, 10)]                                                    # identity, mirror, odd / even quarter turns, flip: either side
PARTNER_STARTS = [50, 0, 100, 0, 77, -20, 120, 10, 60, 140, 0, 99, 33, 5, 149, 64]   # [3]: silent frame 62 of a meets 5 of b


@pytest.mark.parametrize("channels,order,mask_value,affine", [(4, "WYZX", 0.0, False), (4, "WXYZ", -80.0, True),
                                                             (7, "WYZX", -80.0, True), (7, "WXYZ", 0.0, False),
                                                             (8, None, -80.0, False), (8, None, 0.0, True)])
def test_mixed_frames_match_the_restatement_in_float64(gpu_device, channels, order, mask_value, affine):
    """The same mix evaluated in float64 from the device's own fp32 timeline (tests/mix_ref.py, which states the bounds).
    Copied frames, masked elements and zero rows: bit-equal to the augmenting pair (and, without the affine map, to the
    restatement).  Labels: equal to the restatement.  channels = 8: 'logmel' of a microphone array, identity patterns."""
    import seld_native
    dev = gpu_device
    rng = np.random.default_rng(10 * channels + affine)
    iv = 3 if channels == 7 else 0
    spec, mask = _timeline(rng, channels, iv)
    table = _table(channels, order)
    assert np.array_equal(table, mix_ref.channel_table(channels, order or "WYZX"))
    B = len(PAIRS)
    rows = _masked_rows(np.zeros((B, 12), dtype=np.int32), rng)
    rows[4:8, 1:9] = 0                                                               # four windows without masks
    rows[:, 0] = [pa if order else 0 for pa, _ in PAIRS]
    gains = np.asarray([(0.25, 1.0, 4.0)[n % 3] for n in range(B)], dtype=np.float32)
    partners_host = mix_ref.pack_partners(PARTNER_STARTS, [pb if order else 0 for _, pb in PAIRS], gains)
    starts = STARTS + STARTS[::-1]
    partners = seld_native.mix_partners(PARTNER_STARTS, [pb if order else 0 for _, pb in PAIRS], gains, dev)
    assert np.array_equal(partners.cpu().numpy(), partners_host)
    spec_d, mask_d = torch.from_numpy(spec).to(dev), torch.from_numpy(mask).to(dev)
    scale_h = shift_h = scale = shift = None
    if affine:
        scale_h, shift_h, scale, shift = _affine(rng, channels, dev)
    params = seld_native.augment_params(rows, B, WINDOW, dev)
    starts_t = torch.as_tensor(starts)
    out = torch.full((B, WINDOW, channels, 64), float("nan"), device=dev)
    got = seld_native.gather_windows_mix(spec_d, starts_t, WINDOW, params, partners, table, channels, mask_value, iv, out=out,
                                         scale=scale, shift=shift).cpu().numpy()
    got_m = seld_native.gather_windows_mix_mask(mask_d, starts_t, WINDOW, params, partners, I, J).cpu().numpy()
    alone = seld_native.gather_windows_augment(spec_d, starts_t, WINDOW, params, table, channels, mask_value, scale=scale,
                                               shift=shift).cpu().numpy()
    want, tol, computed, floor_ok, want_m, mixed = mix_ref.gather(spec, mask, starts, rows, partners_host, WINDOW, table, iv,
                                                                   channels, mask_value, scale_h, shift_h, I, J)
    assert np.isfinite(got).all() and mixed.any(axis=1).all()
    assert mixed[7, :10].all() and not mixed[7, 10:].any() and not mixed[5, :20].any() and mixed[5, 20:].all()
    assert mixed[9, :10].all() and not mixed[9, 10:].any() and mixed[14].sum() == 1
    assert np.array_equal(got_m, want_m) and want_m.any()
    alone_m = seld_native.gather_windows_permute(mask_d, starts_t, WINDOW, params, I, J).cpu().numpy()
    assert not np.array_equal(got_m[mixed], alone_m[mixed]) and np.array_equal(got_m[~mixed], alone_m[~mixed])
    assert np.array_equal(_bits(got)[~computed], _bits(alone)[~computed])
    if not affine:
        assert np.array_equal(_bits(got)[~computed], _bits(want.astype(np.float32))[~computed])
    assert (got[~computed] == np.float32(mask_value)).any() and not got[7, 10:].any()
    err = np.abs(got.astype(np.float64) - want)
    if affine:                                                       # the floor, seen through the map
        floor_value = np.float32(-100.0) * scale_h + shift_h
        at_floor = np.abs(got - floor_value) <= 2.0 ** -22 * np.abs(floor_value)
    else:
        at_floor = got == -100.0
    ok = (err <= tol) | (floor_ok & at_floor)
    mel = np.zeros(computed.shape, dtype=bool)
    mel[:, :, :channels - iv] = computed[:, :, :channels - iv]
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(computed & (tol > 0), err / tol, 0.0)
    # elements where one or both operands sit at the floor are among the computed ones
    floor_a, both_silent = np.zeros(computed.shape, dtype=bool), np.zeros(computed.shape, dtype=bool)
    for b in range(B):
        for w in np.nonzero(mixed[b])[0]:
            a_row = spec[starts[b] + w][table[rows[b, 0]] & 0x7f][:channels - iv]
            b_row = spec[PARTNER_STARTS[b] + w][table[PAIRS[b][1] if order else 0] & 0x7f][:channels - iv]
            floor_a[b, w, :channels - iv] = (a_row == -100.0) | (b_row == -100.0)
            both_silent[b, w, :channels - iv] = (a_row == -100.0) & (b_row == -100.0)
    floor_a &= computed
    both_silent &= computed
    print(f"C = {channels} {order} affine {affine}: log-mel worst error / bound {ratio[mel].max():.3f} (largest bound "
          f"{tol[mel].max():.2e}), intensity worst error / bound {ratio[computed & ~mel].max() if iv else 0.0:.3f}; "
          f"{int((floor_ok & computed).sum())} elements near the floor, {int((floor_a & computed).sum())} with an operand at -100, "
          f"{int(both_silent.sum())} silent + silent")
    assert ok[computed].all(), float(ratio.max())
    assert floor_a.sum() > 100 and both_silent.sum() > 60 and both_silent[3, 5].any()
    if not affine:                                                   # silence mixed with silence is -100 exactly
        assert (got[both_silent] == -100.0).all()
    # a window's output depends on (src, starts[b], params[b], partners[b]) only: the same windows in another batch
    pick = [9, 2, 2, 15]
    sub = seld_native.gather_windows_mix(spec_d, torch.as_tensor([starts[i] for i in pick]), WINDOW,
                                         seld_native.augment_params(rows[pick], len(pick), WINDOW, dev),
                                         torch.from_numpy(partners_host[pick]).to(dev), table, channels, mask_value, iv,
                                         scale=scale, shift=shift).cpu().numpy()
    assert np.array_equal(_bits(sub), _bits(got[pick]))
    # a device table is trusted no further than its bits: garbage above bit 35 of the second word changes nothing
    hostile = partners_host.copy()
    hostile[:, 1] |= np.int64(0x7A5) << 36
    again = seld_native.gather_windows_mix(spec_d, starts_t, WINDOW, params, torch.from_numpy(hostile).to(dev), table, channels,
                                           mask_value, iv, scale=scale, shift=shift).cpu().numpy()
    again_m = seld_native.gather_windows_mix_mask(mask_d, starts_t, WINDOW, params, torch.from_numpy(hostile).to(dev), I, J)
    assert np.array_equal(_bits(again), _bits(got)) and np.array_equal(again_m.cpu().numpy(), got_m)


# ------------------------------------------------------------------------------------------ 3. entry refusals

GOOD_TABLE = np.tile(np.arange(4, dtype=np.uint8), (16, 1))
BAD_TABLE = GOOD_TABLE.copy()
BAD_TABLE[3, 2] = 4
FEATURES = ("seld_window_gather_mix", "seld_window_gather_mix_standardised")
LABELS = ("seld_window_mix_mask",)


def _cases():
    """(entry point, case, overrides of the good call, expected return code), after tests/test_window_entry_refusals_gpu.py."""
    rows = []
    for name in FEATURES + LABELS:
        pointers = ("src", "starts", "params", "partners", "dst") + (("table",) if name in FEATURES else ())
        rows += [(name, "total_rows = -1", {"total_rows": -1}, INVALID), (name, "B = -1", {"B": -1}, INVALID),
                 (name, "window = 0", {"window": 0}, INVALID), (name, "B = 1, null src", {"src": None}, INVALID),
                 (name, "B = 1, null params", {"params": None}, INVALID),
                 (name, "B = 1, null partners", {"partners": None}, INVALID), (name, "B = 1, null dst", {"dst": None}, INVALID),
                 (name, "B = 0, every pointer null", dict({p: None for p in pointers}, B=0), 0)]
    for name in FEATURES:
        rows += [(name, "iv_channels = 1", {"iv_channels": 1}, UNSUPPORTED), (name, "iv_channels = 4", {"iv_channels": 4}, UNSUPPORTED),
                 (name, "iv_channels = -3", {"iv_channels": -3}, UNSUPPORTED),
                 (name, "iv_channels = 3 with 4 channels", {"iv_channels": 3}, UNSUPPORTED),
                 (name, "iv_channels = 3 with 8 channels", {"iv_channels": 3, "channels": 8, "freq_channels": 8}, UNSUPPORTED),
                 (name, "channels = 65", {"channels": 65}, UNSUPPORTED),
                 (name, "channels = 0", {"channels": 0, "freq_channels": 0}, INVALID),
                 (name, "freq_channels > channels", {"freq_channels": 5}, INVALID),
                 (name, "2^31 chunks in a window", {"window": (1 << 31) // 64}, UNSUPPORTED),
                 (name, "channel table names a channel >= channels", {"table": BAD_TABLE}, INVALID),
                 (name, "B = 0, iv_channels = 1", {"B": 0, "iv_channels": 1}, UNSUPPORTED)]
    rows += [("seld_window_gather_mix_standardised", "B = 1, null scale", {"scale": None}, INVALID),
             ("seld_window_gather_mix_standardised", "B = 1, null shift", {"shift": None}, INVALID)]
    name = "seld_window_mix_mask"
    rows += [(name, "I = 0", {"I": 0}, INVALID), (name, "J = 34", {"J": 34}, UNSUPPORTED),
             (name, "I*J = 20*6", {"I": 20, "J": 6}, UNSUPPORTED), (name, "I*J = 5*4", {"I": 5, "J": 4}, UNSUPPORTED),
             (name, "2^31 chunks in a window", {"window": -(-(1 << 31) // 81)}, UNSUPPORTED)]
    return rows


CASES = _cases()


def _call(lib, name, buf, stream, overrides):
    p = ctypes.c_void_p(buf.data_ptr())
    a = {"src": p, "starts": p, "params": p, "partners": p, "dst": p, "scale": p, "shift": p, "table": GOOD_TABLE, "total_rows": 1,
         "B": 1, "window": 1, "channels": 4, "freq_channels": 4, "iv_channels": 0, "I": 18, "J": 36}
    a.update(overrides)
    table = ctypes.c_void_p(a["table"].ctypes.data) if a["table"] is not None else None
    if name == "seld_window_gather_mix":
        return lib.seld_window_gather_mix(a["src"], a["total_rows"], a["channels"], a["freq_channels"], a["starts"], a["params"],
                                          a["partners"], a["B"], a["window"], table, 0.0, a["iv_channels"], a["dst"], stream)
    if name == "seld_window_gather_mix_standardised":
        return lib.seld_window_gather_mix_standardised(a["src"], a["total_rows"], a["channels"], a["freq_channels"], a["starts"],
                                                 a["params"], a["partners"], a["B"], a["window"], table, 0.0, a["iv_channels"],
                                                 a["scale"], a["shift"], a["dst"], stream)
    return lib.seld_window_mix_mask(a["src"], a["total_rows"], a["I"], a["J"], a["starts"], a["params"], a["partners"], a["B"],
                                    a["window"], a["dst"], stream)


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
    rc = _call(lib, name, buf, stream, overrides)
    print(name, case, rc, lib.seld_last_error())
    assert rc == expected
    if expected:
        assert lib.seld_last_error().startswith(name.encode() + b":")


def test_bindings_refuse_tables_of_the_wrong_kind(gpu_device):
    import seld_native
    dev = gpu_device
    spec = torch.zeros((60, 4, 64), device=dev)
    params = seld_native.augment_params(np.zeros((1, 12), np.int32), 1, WINDOW, dev)
    starts = torch.zeros(1, dtype=torch.int64)
    for bad in (torch.zeros((1, 2), dtype=torch.int64), torch.zeros((1, 2), dtype=torch.int32, device=dev),
                torch.zeros((2, 2), dtype=torch.int64, device=dev), None):
        with pytest.raises(ValueError, match="partners"):
            seld_native.gather_windows_mix(spec, starts, WINDOW, params, bad)
    with pytest.raises(seld_native.SeldNativeError, match="-4"):
        seld_native.gather_windows_mix(spec, starts, WINDOW, params, seld_native.mix_partners([0], [0], [1.0], dev), iv_channels=3)


# ------------------------------------------------------------------------------------------ 4. physical consistency

@pytest.mark.parametrize("order", ["WYZX", "WXYZ"])
def test_mixed_windows_equal_the_windows_of_the_mixed_recording(gpu_device, class_config, order):
    """Dataset A: three band-limited plane-wave clips (300 - 3 000 Hz, 5 000 - 9 000 Hz, 300 - 3 000 Hz), gathered with
    partners one clip further on (sb = sa + 50), gain g, patterns (pa, pb).  Dataset B: built from scratch from the clips
    T_pa(clip_i) + sqrt(g) T_pb(clip_i+1) and the united, transformed metadata.  Labels bit-equal; log-mel within 1e-4 dB and
    intensity vectors within 1e-4 of the float64 oracle on the mixed clips, over the mel bands whose filter lies inside a pass
    band and frames 2 .. 47 of each clip -- the condition under which tests/test_mix_cpu.py shows the definition itself exact
    to 6e-6 dB / 1.1e-5.  Nothing else is left out."""
    dev = gpu_device
    clips = [mix_ref.band_limited_clip_f32(order, n) for n in range(3)]
    rows = [mix_ref.clip_rows(n) for n in range(3)]
    ds_a = _dataset(class_config, dev, "logmel_iv", order, clips, rows)
    assert ds_a.total_frames == TOTAL and len(ds_a) == 15 and ds_a.window_length_frames == WINDOW and ds_a.n_channels == 7
    idx = [0, 1, 2, 3, 4, 5]                                          # starts 0 .. 50: every partner row inside the timeline
    starts = ds_a.window_starts[idx]
    partner = np.asarray(idx) + WINDOW // HOP
    assert np.array_equal(ds_a.window_starts[partner], starts + WINDOW) and starts[-1] + 2 * WINDOW == TOTAL
    plain_s, plain_m = (t.cpu().numpy() for t in ds_a.device_batch(idx))
    bands = list(mix_ref.LISTED_BANDS)
    keep = np.zeros(TOTAL, dtype=bool)                                # frames 2 .. 47 of the two mixed clips
    for clip in range(2):
        keep[clip * 50 + 2:clip * 50 + 48] = True
    worst_db = worst_iv = 0.0
    for pa, pb, g in ((0, 0, 1.0), (10, 5, 0.25), (7, 12, 4.0)):
        ta, tb = rotate_ref.split(pa), rotate_ref.split(pb)
        sa_, sb_ = (ta[0], ta[1] * (J // 4), ta[2]), (tb[0], tb[1] * (J // 4), tb[2])
        mixed_clips, mixed_rows = [], []
        for n in range(3):
            a = rotate_ref.pcm_transformed(clips[n].numpy(), *sa_, order)
            if n < 2:
                a = a + np.sqrt(g) * rotate_ref.pcm_transformed(clips[n + 1].numpy(), *sb_, order)
                mixed_rows.append(mix_ref.united_rows(rotate_ref.rows_transformed(rows[n], *sa_),
                                                      rotate_ref.rows_transformed(rows[n + 1], *sb_)))
            else:
                mixed_rows.append(rotate_ref.rows_transformed(rows[n], *sa_))
            mixed_clips.append(torch.from_numpy(a.astype(np.float32)))
        ds_b = _dataset(class_config, dev, "logmel_iv", order, mixed_clips, mixed_rows)
        params = np.zeros((len(idx), 12), dtype=np.int32)
        params[:, 0] = pa
        mix = (partner, np.full(len(idx), pb, dtype=np.int32), np.full(len(idx), g, dtype=np.float32))
        aug_s, aug_m = (t.cpu().numpy() for t in ds_a.device_batch(idx, augment=params, mix=mix))
        _, ref_m = (t.cpu().numpy() for t in ds_b.device_batch(idx))
        assert np.array_equal(aug_m, ref_m) and ref_m.any() and not np.array_equal(aug_m, plain_m), (pa, pb, g)
        # float64 oracle on the mixed clips as they were fed (fp32 samples), cropped and concatenated like the timeline
        ref_tm = np.concatenate([np.concatenate([ofeat.logmel_f64(c.numpy().astype(np.float64)),
                                                 ofeat.foa_intensity_f64(c.numpy().astype(np.float64))])[:, :, :50].transpose(2, 0, 1)
                                 for c in mixed_clips])                              # [150, 7, 64]
        for b, start in enumerate(starts):
            frames = np.arange(start, start + WINDOW)
            sel = keep[frames]
            err = np.abs(aug_s[b][sel].astype(np.float64) - ref_tm[frames[sel]])[:, :, bands]
            worst_db, worst_iv = max(worst_db, float(err[:, :4].max())), max(worst_iv, float(err[:, 4:].max()))
        print(f"order {order} (pa, pb, g) = ({pa}, {pb}, {g}): worst log-mel error so far {worst_db:.3e} dB, intensity {worst_iv:.3e} "
              f"(intensity range {np.abs(ref_tm[keep][:, 4:][:, :, bands]).max():.2f})")
        assert not np.array_equal(_bits(aug_s), _bits(plain_s))
        assert worst_db <= 1e-4 and worst_iv <= 1e-4, (pa, pb, g, worst_db, worst_iv)


# ------------------------------------------------------------------------------------------ 5. training path

def test_feed_refusals(gpu_device, class_config):
    import dataset
    import seld_augment
    import trainer
    dev = gpu_device
    clips = [rotate_ref.plane_wave_clip("WYZX", n) for n in range(3)]
    rows = [rotate_ref.clip_rows() for _ in clips]
    ds = _dataset(class_config, dev, "logmel", "WYZX", clips, rows)
    idx = [0, 4, 14]
    mix = (np.asarray([3, -1, 0]), np.zeros(3, np.int32), np.asarray([1.0, 0.0, 2.0], np.float32))
    with pytest.raises(ValueError, match="augment rows"):
        ds.device_batch(idx, mix=mix)
    with pytest.raises(ValueError, match="partner outside"):
        ds.device_batch(idx, augment=seld_augment.identity_rows(3), mix=(np.asarray([3, -1, 15]), mix[1], mix[2]))
    got_s, got_m = ds.device_batch(idx, augment=seld_augment.identity_rows(3), mix=mix)
    plain_s, plain_m = ds.device_batch(idx)
    assert torch.equal(got_s[1].view(torch.int32), plain_s[1].view(torch.int32)) and not torch.equal(got_s[0], plain_s[0])
    assert torch.equal(got_m[1].view(torch.int16), plain_m[1].view(torch.int16))
    class_config.AUGMENT_ROTATE = True
    with_terms = dataset.SELDDataset.from_pcm(clips, rows, device=dev)
    class_config.AUGMENT_ROTATE = False
    with pytest.raises(ValueError, match="rotating gathers"):
        with_terms.device_batch(idx, augment=seld_augment.identity_rows(3), mix=mix)
    cfg = trainer.config
    shadowed = "FEATURE_SET" in vars(cfg)                 # an earlier test may have left an instance attribute over the class's
    shadow = vars(cfg).get("FEATURE_SET")
    try:
        cfg.FEATURE_SET = "logmel"
        class_config.AUGMENT_MIX_PROB = 0.5
        assert isinstance(trainer.make_feed(DataLoader(ds, batch_size=2, shuffle=False), dev, 0, 1), trainer.DeviceFeed)
        with pytest.raises(ValueError, match="AUGMENT_MIX_PROB"):
            trainer.make_feed(DataLoader(with_terms, batch_size=2, shuffle=False), dev, 0, 1)
        class_config.AUGMENT_ROTATE = True
        with pytest.raises(ValueError, match="cannot be combined with AUGMENT_ROTATE"):
            trainer.make_feed(DataLoader(with_terms, batch_size=2, shuffle=False), dev, 0, 1)
        class_config.AUGMENT_ROTATE = False
        for feature_set in ("logmel_gcc", "logmel_nipd"):
            cfg.FEATURE_SET = feature_set
            with pytest.raises(ValueError, match="AUGMENT_MIX_PROB is defined for power features"):
                trainer.make_feed(DataLoader(ds, batch_size=2, shuffle=False), dev, 0, 1)
    finally:
        if shadowed:
            cfg.FEATURE_SET = shadow
        else:
            del cfg.FEATURE_SET


def test_training_with_the_mix_is_reproducible_and_evaluation_is_untouched(gpu_device, class_config, tmp_path):
    """Two train_model runs (2 epochs, small CRNN, captured steps, SEED set) with AUGMENT_MIX_PROB = 0.5 give identical loss
    histories, which differ from the run with it off; a window's batch differs between epoch 1 and epoch 2 wherever its
    partner does; the evaluation feed of the same process returns un-mixed windows."""
    import seld_augment
    import trainer
    cfg = trainer.config
    names = ("MODEL_TYPE", "CRNN_CNN_CHANNELS", "CRNN_RNN_HIDDEN", "CRNN_DROPOUT", "NUM_EPOCHS", "BATCH_SIZE", "SEED",
             "OUTPUT_PATH", "CHECKPOINT_PATH", "GRAPH_STEP", "DEVICE_FEED")
    saved = {k: getattr(cfg, k) for k in names}
    saved_det = torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark
    shadowed = "FEATURE_SET" in vars(cfg)                 # an earlier test may have left an instance attribute over the class's
    shadow = vars(cfg).get("FEATURE_SET")
    try:
        cfg.FEATURE_SET = "logmel_iv"
        torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = True, False
        cfg.MODEL_TYPE, cfg.CRNN_CNN_CHANNELS, cfg.CRNN_RNN_HIDDEN, cfg.CRNN_DROPOUT = "crnn", [8, 8, 16, 16], 16, 0.0
        cfg.NUM_EPOCHS, cfg.BATCH_SIZE, cfg.SEED, cfg.GRAPH_STEP, cfg.DEVICE_FEED = 2, 4, 11, True, True
        cfg.OUTPUT_PATH, cfg.CHECKPOINT_PATH = tmp_path / "outputs", tmp_path / "checkpoints"
        cfg.OUTPUT_PATH.mkdir()
        cfg.CHECKPOINT_PATH.mkdir()
        clips = [rotate_ref.plane_wave_clip("WYZX", n) for n in range(18)]
        rows = [mix_ref.clip_rows(n % 4) for n in range(18)]
        train_ds = _dataset(class_config, gpu_device, "logmel_iv", "WYZX", clips[:12], rows[:12], window=250, hop=50)
        test_ds = _dataset(class_config, gpu_device, "logmel_iv", "WYZX", clips[12:], rows[12:], window=250, hop=50)
        assert len(train_ds) == 12 and train_ds.rot_tm is None
        train_loader = DataLoader(train_ds, batch_size=cfg.BATCH_SIZE, shuffle=True)
        test_loader = DataLoader(test_ds, batch_size=cfg.BATCH_SIZE, shuffle=False)

        def run(prob):
            class_config.AUGMENT_MIX_PROB = prob
            assert trainer.graph_step_enabled(gpu_device, 1)
            for old in cfg.CHECKPOINT_PATH.glob("*.pth"):
                old.unlink()
            _, history = trainer.train_model(train_loader=train_loader, test_loader=test_loader, device=gpu_device)
            assert history["total_epochs"] == 2 and history["config"]["batch_source"] == "DeviceFeed"
            return history["train_losses"], history["test_losses"]

        first, second, off = run(0.5), run(0.5), run(0.0)
        print("mixed:", first, "again:", second, "switch off:", off)
        assert np.isfinite(first[0]).all() and np.isfinite(first[1]).all()
        assert first == second
        assert first[0] != off[0]

        class_config.AUGMENT_MIX_PROB = 0.5
        n = len(train_ds)
        ordered = DataLoader(train_ds, batch_size=n, shuffle=False)
        feed = trainer.make_feed(ordered, gpu_device, 0, 1)
        e1 = [t.clone() for t in next(iter(feed.batches(1, augment=True)))]
        e1_again = [t.clone() for t in next(iter(feed.batches(1, augment=True)))]
        e2 = [t.clone() for t in next(iter(feed.batches(2, augment=True)))]
        assert torch.equal(e1[0].view(torch.int32), e1_again[0].view(torch.int32))
        assert torch.equal(e1[1].view(torch.int16), e1_again[1].view(torch.int16))
        plain = train_ds.device_batch(list(range(n)))
        d1, d2 = (seld_augment.draw_mix(feed.seed, e, np.arange(n), cfg, n) for e in (1, 2))
        changed = 0
        for w in range(n):
            same_draw = d1[0][w] == d2[0][w] and d1[2][w] == d2[2][w]
            if not same_draw:
                changed += 1
                assert not torch.equal(e1[0][w], e2[0][w]), w
            for draw_, got in ((d1, e1), (d2, e2)):
                if draw_[0][w] < 0:                                   # no partner: the plain window, bit for bit
                    assert torch.equal(got[0][w].view(torch.int32), plain[0][w].view(torch.int32)), w
                    assert torch.equal(got[1][w].view(torch.int16), plain[1][w].view(torch.int16)), w
                else:
                    assert not torch.equal(got[0][w], plain[0][w]), w
        assert changed >= 3 and (d1[0] >= 0).any() and (d1[0] < 0).any()
        for got in (next(iter(feed.batches(1))), next(iter(feed.batches(0, augment=False)))):
            assert torch.equal(got[0].view(torch.int32), plain[0].view(torch.int32))
            assert torch.equal(got[1].view(torch.int16), plain[1].view(torch.int16))
        small = trainer.make_feed(DataLoader(train_ds, batch_size=5, shuffle=False), gpu_device, 0, 1)
        parts = [s.clone() for s, _ in small.batches(1, augment=True)]
        assert torch.equal(torch.cat(parts).view(torch.int32), e1[0].view(torch.int32))
        results_on = trainer.test_model(test_loader=test_loader, model_path=cfg.CHECKPOINT_PATH / "best_model.pth",
                                        device=gpu_device, num_visualizations=1, save_visualizations=False)
        class_config.AUGMENT_MIX_PROB = 0.0
        results_off = trainer.test_model(test_loader=test_loader, model_path=cfg.CHECKPOINT_PATH / "best_model.pth",
                                         device=gpu_device, num_visualizations=1, save_visualizations=False)
        assert results_on["test_loss"] == results_off["test_loss"]
    finally:
        torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = saved_det
        for k, v in saved.items():
            setattr(cfg, k, v)
        if shadowed:
            cfg.FEATURE_SET = shadow
        else:
            del cfg.FEATURE_SET
