"""GPU tests of the channel swap for microphone-array features (csrc/micswap.hip, seld_augment.py, dataset.py; DESIGN.md
section 25): the gather bit for bit against the numpy restatement of tests/mic_swap_ref.py, pattern 0 against the
augmenting and the plain gather, the physics (features of the channel-permuted recording), what the entry points refuse,
one graph capture, and the dataset / test-time-augmentation path.  Shapes: a 37-row timeline, 16-frame windows."""
import ctypes

import numpy as np
import pytest
import torch

import mic_swap_ref as ref
import nipd_ref
from oracle import features as ofeat
from oracle import labels as olab

pytestmark = pytest.mark.gpu

TOTAL, WINDOW = 37, 16
STARTS = [-5, 0, 11, 30, 37, 21]        # begins before the timeline, inside, runs past it, wholly outside
SENTINEL_BITS = 0x7FC12345              # a NaN payload nothing computes
MASK_VALUE = -7.5
INVALID, UNSUPPORTED = -1, -4
ARRAYS = {"tetra": ref.tetrahedron(), "cube": ref.cube()}
CONFIG_NAMES = ("FEATURE_SET", "MIC_POSITIONS", "AUGMENT_SPATIAL", "AUGMENT_ROTATE", "AUGMENT_TIME_MASKS", "AUGMENT_TIME_MASK_MAX",
                "AUGMENT_FREQ_MASKS", "AUGMENT_FREQ_MASK_MAX", "AUGMENT_MASK_VALUE", "AUGMENT_MIX_PROB", "AUGMENT_MIX_GAIN_DB",
                "WINDOW_LENGTH", "HOP_LENGTH", "SELD_TTA_PATTERNS")


def _bits(a):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a).view(np.int32 if a.dtype == np.float32 else a.dtype)


def _channels(mics, kind):
    return mics + mics * (mics - 1) // 2 if kind == "gcc" else 2 * mics - 1


def _timeline(channels, seed):
    """float32 [TOTAL, channels, 64]: random values with some -0.0 and some exact zeros."""
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(TOTAL, channels, 64)).astype(np.float32)
    pick = rng.random(x.shape)
    x[pick < 0.03] = 0.0
    x[(pick >= 0.03) & (pick < 0.06)] = -0.0
    assert np.signbit(x[x == 0]).any() and not np.signbit(x[x == 0]).all()
    return x


def _rows(patterns, masks):
    """One row per (pattern, start): int32 [P * 6, 12], and the matching starts."""
    rows = np.zeros((len(patterns) * len(STARTS), 12), dtype=np.int32)
    rows[:, 0] = np.repeat(patterns, len(STARTS))
    if masks:
        rows[:, 1:5] = (2, 3, 9, 7)      # frames 2..4 and 9..15
        rows[:, 5:9] = (0, 5, 61, 3)     # bins 0..4 and 61..63
    return rows, np.tile(STARTS, len(patterns)).astype(np.int64)


def _affine(channels, seed, dev):
    """Arbitrary scales of either sign and arbitrary shifts (the restatement's fma32 is exact for any)."""
    rng = np.random.default_rng(seed)
    scale = (rng.uniform(0.1, 8.0, size=(channels, 64)) * rng.choice([-1.0, 1.0], size=(channels, 64))).astype(np.float32)
    shift = rng.normal(size=(channels, 64)).astype(np.float32)
    return scale, shift, torch.from_numpy(scale).to(dev), torch.from_numpy(shift).to(dev)


def _sentinel(shape, dev):
    return torch.full(shape, SENTINEL_BITS, dtype=torch.int32, device=dev).view(torch.float32)


@pytest.mark.parametrize("affine", [False, True])
@pytest.mark.parametrize("kind", ["gcc", "nipd"])
@pytest.mark.parametrize("array", ["tetra", "cube"])
def test_bit_exact_against_the_restatement(gpu_device, array, kind, affine):
    import seld_augment
    import seld_native
    positions = ARRAYS[array]
    mics, channels = len(positions), _channels(len(positions), kind)
    assert channels == {("tetra", "gcc"): 10, ("tetra", "nipd"): 7, ("cube", "gcc"): 36, ("cube", "nipd"): 15}[(array, kind)]
    valid = ref.valid_patterns(positions)
    assert len(valid) == (8 if array == "tetra" else 16)
    perm = seld_augment.mic_permutations(positions)
    x = _timeline(channels, 100 + channels)
    src = torch.from_numpy(x).to(gpu_device)
    freq_channels = mics if kind == "gcc" else channels
    scale = shift = scale_d = shift_d = None
    if affine:
        scale, shift, scale_d, shift_d = _affine(channels, 7, gpu_device)
    for masks in (False, True):
        rows, starts = _rows(valid, masks)
        params = seld_native.augment_params(rows, len(rows), WINDOW, gpu_device)
        out = _sentinel((len(rows), WINDOW, channels, 64), gpu_device)
        got = seld_native.gather_windows_mic(src, torch.from_numpy(starts), WINDOW, params, perm, "logmel_" + kind,
                                             freq_channels, MASK_VALUE, out=out, scale=scale_d, shift=shift_d)
        assert got is out
        want, _ = ref.gather(x, None, starts, rows, WINDOW, positions, kind, freq_channels, MASK_VALUE, scale, shift)
        got_bits = _bits(got)
        assert not (got_bits == SENTINEL_BITS).any()
        assert np.array_equal(got_bits, _bits(want)), (array, kind, affine, masks)
        # the swap really happens, and the window wholly outside the timeline is +0.0 bits
        outside = [i for i, s in enumerate(starts) if s >= TOTAL]
        assert len(outside) == len(valid) and not got_bits[outside].any()
        moved = rows[:, 0] != 0
        identity_rows = np.zeros_like(rows)
        identity_rows[:, 1:] = rows[:, 1:]
        same, _ = ref.gather(x, None, starts, identity_rows, WINDOW, positions, kind, freq_channels, MASK_VALUE, scale, shift)
        assert not np.array_equal(_bits(want)[moved], _bits(same)[moved])


@pytest.mark.parametrize("kind", ["gcc", "nipd"])
def test_pattern_zero_and_invalid_patterns_are_the_other_gathers(gpu_device, kind):
    import seld_augment
    import seld_native
    positions = ARRAYS["tetra"]
    channels = _channels(4, kind)
    perm = seld_augment.mic_permutations(positions)
    x = _timeline(channels, 31)
    src = torch.from_numpy(x).to(gpu_device)
    freq_channels = 4 if kind == "gcc" else channels
    identity = np.tile(np.arange(channels, dtype=np.uint8), (16, 1))
    # pattern 0 and the patterns that are no symmetry of the tetrahedron: all the identity transform
    for masks in (False, True):
        rows, starts = _rows([0, 1, 2, 15], masks)
        params = seld_native.augment_params(rows, len(rows), WINDOW, gpu_device)
        starts_t = torch.from_numpy(starts)
        got = seld_native.gather_windows_mic(src, starts_t, WINDOW, params, perm, "logmel_" + kind, freq_channels, MASK_VALUE)
        other = seld_native.gather_windows_augment(src, starts_t, WINDOW, params, identity, freq_channels, MASK_VALUE)
        assert np.array_equal(_bits(got), _bits(other))
        if not masks:
            assert np.array_equal(_bits(got), _bits(seld_native.gather_windows(src, starts_t, WINDOW)))


# ------------------------------------------------------------------------------------------ the physics

SAMPLES = 12000                      # 0.5 s
SPEED = 343.0


def _band_noise(rng, lo_hz, hi_hz):
    spectrum = np.fft.rfft(rng.normal(size=SAMPLES))
    f = np.fft.rfftfreq(SAMPLES, 1.0 / 24000.0)
    spectrum[(f < lo_hz) | (f > hi_hz)] = 0.0
    return spectrum


def _array_recording(positions, directions, bands, seed, sensor_noise):
    """float32 [C, SAMPLES]: plane waves of band-limited noise from ``directions`` (unit vectors), microphone j hearing a
    source (r_j . d) / c seconds EARLY -- a phase ramp on the source's spectrum in float64 -- plus independent sensor noise."""
    rng = np.random.default_rng(seed)
    f = np.fft.rfftfreq(SAMPLES, 1.0 / 24000.0)
    pcm = np.zeros((len(positions), SAMPLES))
    for d, (lo, hi) in zip(directions, bands):
        spectrum = _band_noise(rng, lo, hi)
        for j, r in enumerate(positions):
            tau = -float(np.dot(r, d)) / SPEED
            pcm[j] += np.fft.irfft(spectrum * np.exp(-2j * np.pi * f * tau), n=SAMPLES)
    pcm *= 0.1 / np.abs(pcm).max()
    pcm += sensor_noise * rng.normal(size=pcm.shape)
    return pcm.astype(np.float32)


def test_transform_then_extract_equals_extract_then_transform_gcc(gpu_device):
    """'logmel_gcc' of the tetrahedron: the gather of the recording's features under p against the features of the
    recording with its channels permuted by sigma_p.  Compared: everything but the first and the last frame and lag index 0
    of the reversed pairs (lag +32 is not stored)."""
    import seld_augment
    import seld_native
    positions = ARRAYS["tetra"]
    directions = [ref.unit(25.0, 10.0), ref.unit(-110.0, -40.0)]
    pcm = _array_recording(positions, directions, [(200.0, 9000.0), (400.0, 6000.0)], 17, 1e-4)
    perm = seld_augment.mic_permutations(positions)
    stored = seld_native.spatial_features(torch.from_numpy(pcm).to(gpu_device), "logmel_gcc")          # [F, 10, 64]
    frames = int(stored.shape[0])
    assert stored.shape[1:] == (10, 64) and frames == 26
    pairs = [(a, b) for a in range(4) for b in range(a + 1, 4)]
    for p in ref.valid_patterns(positions):
        sig = ref.TETRA_SIGMA[p]
        swapped = torch.from_numpy(np.ascontiguousarray(pcm[sig])).to(gpu_device)
        want = seld_native.spatial_features(swapped, "logmel_gcc").cpu().numpy()
        rows = np.zeros((1, 12), dtype=np.int32)
        rows[0, 0] = p
        params = seld_native.augment_params(rows, 1, frames, gpu_device)
        got = seld_native.gather_windows_mic(stored, torch.zeros(1, dtype=torch.int64), frames, params, perm, "logmel_gcc",
                                             4, 0.0)[0].cpu().numpy()
        compared = np.ones(got.shape, dtype=bool)
        compared[0] = compared[-1] = False
        reversed_pairs = [n for n, (a, b) in enumerate(pairs) if sig[a] > sig[b]]
        for n in reversed_pairs:
            compared[:, 4 + n, 0] = False
        excluded = 2 * 10 * 64 + (frames - 2) * len(reversed_pairs)
        assert int((~compared).sum()) == excluded
        assert np.array_equal(_bits(got[:, :4])[compared[:, :4]], _bits(want[:, :4])[compared[:, :4]]), p     # log-mel: bit-equal
        err = np.abs(got[:, 4:].astype(np.float64) - want[:, 4:])[compared[:, 4:]].max()
        print(f"pattern {p}: {len(reversed_pairs)} reversed pairs, max |GCC difference| = {err:.3e}")
        assert err <= 2e-4, (p, err)
        if p:
            assert np.abs(got[:, 4:] - stored.cpu().numpy()[:, 4:]).max() > 0.05              # and it is not the identity


def test_transform_then_extract_equals_extract_then_transform_nipd(gpu_device):
    """'logmel_nipd' of the tetrahedron, one source and no sensor noise, so that no phase difference wraps below
    NIPD_MAX_HZ (checked here in float64): the NIPD rule then reproduces the features of the permuted recording.
    Compared: everything but the first and the last frame."""
    import seld_augment
    import seld_native
    positions = ARRAYS["tetra"]
    pcm = _array_recording(positions, [ref.unit(70.0, 20.0)], [(20.0, 11000.0)], 23, 0.0)
    # no wrap: every microphone pair's phase difference in the NIPD range stays clear of +-pi
    phi = nipd_ref.pcm_phase(pcm)[:, 1:-1][..., nipd_ref.in_range(50.0, 2000.0)]                      # [3, F - 2, bins]
    widest = max(np.abs(phi).max(), max(np.abs(phi[a] - phi[b]).max() for a in range(3) for b in range(a)))
    assert widest < np.pi - 0.3, widest
    perm = seld_augment.mic_permutations(positions)
    stored = seld_native.spatial_features(torch.from_numpy(pcm).to(gpu_device), "logmel_nipd", nipd_min_hz=50.0,
                                          nipd_max_hz=2000.0, sound_speed=SPEED)
    frames = int(stored.shape[0])
    assert stored.shape[1:] == (7, 64) and frames == 26
    for p in ref.valid_patterns(positions):
        sig = ref.TETRA_SIGMA[p]
        swapped = torch.from_numpy(np.ascontiguousarray(pcm[sig])).to(gpu_device)
        want = seld_native.spatial_features(swapped, "logmel_nipd", nipd_min_hz=50.0, nipd_max_hz=2000.0,
                                            sound_speed=SPEED).cpu().numpy()
        rows = np.zeros((1, 12), dtype=np.int32)
        rows[0, 0] = p
        params = seld_native.augment_params(rows, 1, frames, gpu_device)
        got = seld_native.gather_windows_mic(stored, torch.zeros(1, dtype=torch.int64), frames, params, perm, "logmel_nipd",
                                             7, 0.0)[0].cpu().numpy()
        compared = np.ones(got.shape, dtype=bool)
        compared[0] = compared[-1] = False
        assert int((~compared).sum()) == 2 * 7 * 64
        assert np.array_equal(_bits(got[:, :4])[compared[:, :4]], _bits(want[:, :4])[compared[:, :4]]), p
        err = np.abs(got[:, 4:].astype(np.float64) - want[:, 4:])[compared[:, 4:]].max()
        print(f"pattern {p}: sigma(0) = {sig[0]}, max |NIPD difference| = {err:.3e} m")
        assert err <= 3e-4, (p, err)
        if sig[0] == 0:
            assert np.array_equal(_bits(got[:, 4:]), _bits(stored.cpu().numpy()[:, 4:][:, [s - 1 for s in sig[1:]]]))
    assert np.abs(stored.cpu().numpy()[1:-1, 4:]).max() > 0.01                                       # centimetres of path


# ------------------------------------------------------------------------------------------ the entry points

def _call(lib, affine, src, total_rows, mics, kind, freq_channels, starts, params, B, window, perm, dst, scale=None, shift=None):
    import seld_native
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    perm_p = None if perm is None else ctypes.c_void_p(perm.ctypes.data)
    head = (p(src), total_rows, mics, kind, freq_channels, p(starts), p(params), B, window, perm_p, 0.0)
    stream = seld_native._stream_ptr(dst.device)
    if affine:
        return lib.seld_window_gather_mic_standardised(*head, p(scale), p(shift), p(dst), stream)
    return lib.seld_window_gather_mic(*head, p(dst), stream)


@pytest.mark.parametrize("affine", [False, True])
def test_refusals_and_their_order(gpu_device, affine):
    import seld_augment
    import seld_native
    lib = seld_native.load_library()
    seld_native.ensure_init(gpu_device)
    perm = seld_augment.mic_permutations(ARRAYS["tetra"])
    src = torch.from_numpy(_timeline(10, 5)).to(gpu_device)
    starts = torch.tensor([0, 30], dtype=torch.int64, device=gpu_device)
    params = torch.zeros((2, 12), dtype=torch.int32, device=gpu_device)
    params[1, 0] = 9
    scale, shift = (torch.ones((10, 64), device=gpu_device), torch.zeros((10, 64), device=gpu_device)) if affine else (None, None)
    dst = _sentinel((2, WINDOW, 10, 64), gpu_device)
    good = dict(src=src, total_rows=TOTAL, mics=4, kind=0, freq_channels=4, starts=starts, params=params, B=2, window=WINDOW,
                perm=perm, dst=dst, scale=scale, shift=shift)
    not_a_permutation = perm.copy()
    not_a_permutation[9] = (1, 1, 3, 2)
    half_absent = perm.copy()
    half_absent[3] = (-1, -1, 0, 1)
    moved_first = perm.copy()
    moved_first[0] = (1, 0, 3, 2)
    absent_first = perm.copy()
    absent_first[0] = -1
    both = not_a_permutation.copy()                                 # a bad row 9 AND a moved row 0: the rows are looked at first
    both[0] = (1, 0, 3, 2)
    cases = [(dict(mics=1), INVALID, "bad extents"), (dict(mics=9), INVALID, "bad extents"),
             (dict(kind=2), INVALID, "bad extents"), (dict(kind=-1), INVALID, "bad extents"),
             (dict(freq_channels=-1), INVALID, "bad extents"), (dict(freq_channels=11), INVALID, "bad extents"),
             (dict(kind=1, freq_channels=8), INVALID, "bad extents"),                  # 2C - 1 = 7 channels
             (dict(total_rows=-1), INVALID, "bad extents"), (dict(window=0), INVALID, "bad extents"),
             (dict(perm=not_a_permutation), INVALID, "neither a permutation"),
             (dict(perm=half_absent), INVALID, "neither a permutation"),
             (dict(perm=moved_first), INVALID, "row 0"), (dict(perm=absent_first), INVALID, "row 0"),
             (dict(window=(1 << 31) // 160 + 1), UNSUPPORTED, "window too large"),
             (dict(src=None), INVALID, "null pointer"), (dict(starts=None), INVALID, "null pointer"),
             (dict(params=None), INVALID, "null pointer"), (dict(perm=None), INVALID, "null pointer"),
             # the order: extents before the table, the table before the window, the window before the pointers
             (dict(mics=9, perm=not_a_permutation, src=None), INVALID, "bad extents"),
             (dict(perm=not_a_permutation, window=(1 << 31) // 160 + 1, src=None), INVALID, "neither a permutation"),
             (dict(perm=both), INVALID, "neither a permutation"),
             (dict(window=(1 << 31) // 160 + 1, src=None), UNSUPPORTED, "window too large")]
    if affine:
        cases += [(dict(scale=None), INVALID, "null pointer"), (dict(shift=None), INVALID, "null pointer")]
    name = "seld_window_gather_mic_standardised" if affine else "seld_window_gather_mic"
    for change, code, text in cases:
        rc = _call(lib, affine, **{**good, **change})
        message = (lib.seld_last_error() or b"").decode()
        assert rc == code, (change.keys(), rc, message)
        assert message.startswith(name + ":") and text in message, (change.keys(), message)
    torch.cuda.synchronize(gpu_device)
    assert (_bits(dst) == SENTINEL_BITS).all()                      # nothing was written
    # B = 0 returns before any pointer is looked at
    assert _call(lib, affine, **{**good, "B": 0, "src": None, "perm": None}) == 0
    assert (_bits(dst) == SENTINEL_BITS).all()
    # the same arguments, corrected, run
    assert _call(lib, affine, **good) == 0
    torch.cuda.synchronize(gpu_device)
    tables = (np.ones((10, 64), np.float32), np.zeros((10, 64), np.float32)) if affine else (None, None)   # (-0.0 -> +0.0)
    want, _ = ref.gather(src.cpu().numpy(), None, [0, 30], params.cpu().numpy(), WINDOW, ARRAYS["tetra"], "gcc", 4, 0.0, *tables)
    assert np.array_equal(_bits(dst), _bits(want))


def test_python_entry_refuses_a_source_of_another_shape(gpu_device):
    import seld_augment
    import seld_native
    perm = seld_augment.mic_permutations(ARRAYS["tetra"])
    params = torch.zeros((1, 12), dtype=torch.int32, device=gpu_device)
    starts = torch.zeros(1, dtype=torch.int64)
    src = torch.zeros((TOTAL, 9, 64), device=gpu_device)
    with pytest.raises(ValueError, match="10 feature channels"):
        seld_native.gather_windows_mic(src, starts, WINDOW, params, perm, "logmel_gcc")
    with pytest.raises(ValueError, match="kind"):
        seld_native.gather_windows_mic(src, starts, WINDOW, params, perm, "logmel_iv")
    with pytest.raises(ValueError, match="mic_perm"):
        seld_native.gather_windows_mic(src, starts, WINDOW, params, perm[:8], "logmel_gcc")


def test_graph_capture_and_replay(gpu_device):
    import seld_augment
    import seld_native
    positions = ARRAYS["cube"]
    perm = seld_augment.mic_permutations(positions)
    x = _timeline(36, 77)
    src = torch.from_numpy(x).to(gpu_device)
    rows, starts = _rows([5, 12], True)
    params = seld_native.augment_params(rows, len(rows), WINDOW, gpu_device)
    starts_d = torch.from_numpy(starts).to(gpu_device)
    eager = seld_native.gather_windows_mic(src, starts_d, WINDOW, params, perm, "logmel_gcc", 8, MASK_VALUE)
    out = _sentinel(tuple(eager.shape), gpu_device)
    torch.cuda.synchronize(gpu_device)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        seld_native.gather_windows_mic(src, starts_d, WINDOW, params, perm, "logmel_gcc", 8, MASK_VALUE, out=out)
    out.copy_(_sentinel(tuple(eager.shape), gpu_device))            # whatever the capture wrote: the replay must write it all
    graph.replay()
    torch.cuda.synchronize(gpu_device)
    assert np.array_equal(_bits(out), _bits(eager))


# ------------------------------------------------------------------------------------------ dataset and trainer

@pytest.fixture
def class_config():
    """Switches are class attributes (config.py is edited in place upstream; dataset.py and trainer.py each hold an instance)."""
    from config import Config
    saved = {k: getattr(Config, k) for k in CONFIG_NAMES}
    yield Config
    for k, v in saved.items():
        setattr(Config, k, v)


def _array_dataset(Config, dev, feature_set, positions="tetra_starss"):
    import dataset
    Config.FEATURE_SET, Config.MIC_POSITIONS = feature_set, positions
    Config.WINDOW_LENGTH, Config.HOP_LENGTH = 20 * 480, 10 * 480
    clips = [ofeat.synth_pcm(700 + i, 4, 24000 + 333 * i, "noise") for i in range(2)]
    rows = [olab.synth_metadata(700 + i, meta_frames=10) for i in range(2)]
    return dataset.SELDDataset.from_pcm(clips, rows, device=dev)


@pytest.mark.parametrize("feature_set", ["logmel_gcc", "logmel_nipd", "logmel"])
def test_dataset_batches_equal_the_restatement(gpu_device, class_config, monkeypatch, feature_set):
    import seld_augment
    import seld_native
    ds = _array_dataset(class_config, gpu_device, feature_set)
    kind = feature_set.replace("logmel_", "")
    channels = {"gcc": 10, "nipd": 7, "logmel": 4}[kind]
    assert ds.n_channels == channels and ds.window_length_frames == 20 and ds.mic_array.shape == (4, 3)
    class_config.AUGMENT_SPATIAL = True
    class_config.AUGMENT_TIME_MASKS, class_config.AUGMENT_TIME_MASK_MAX = 2, 6
    class_config.AUGMENT_FREQ_MASKS, class_config.AUGMENT_FREQ_MASK_MAX = 1, 9
    class_config.AUGMENT_MASK_VALUE = MASK_VALUE
    idx = list(range(len(ds))) + [1, 0]
    rows = seld_augment.draw(3, 1, idx, class_config, window=20)
    assert set(rows[:, 0].tolist()) <= {0, 3, 4, 7, 9, 10, 13, 14} and len(set(rows[:, 0].tolist())) > 2
    spec_tm, mask_tm = ds.spec_tm.cpu().numpy(), ds.mask_tm.cpu().numpy()
    starts = ds.window_starts[np.asarray(idx)]
    freq_channels = 4 if kind == "gcc" else channels
    calls = []
    for name in ("gather_windows_mic", "gather_windows_augment"):
        real = getattr(seld_native, name)
        monkeypatch.setattr(seld_native, name, lambda *a, _real=real, _name=name, **k: (calls.append(_name), _real(*a, **k))[1])
    spec, mask = ds.device_batch(idx, augment=rows)
    want_spec, want_mask = ref.gather(spec_tm, mask_tm, starts, rows, 20, ref.tetrahedron(), kind, freq_channels, MASK_VALUE)
    assert np.array_equal(_bits(spec), _bits(want_spec)) and np.array_equal(mask.cpu().numpy(), want_mask)
    assert calls == ["gather_windows_augment" if kind == "logmel" else "gather_windows_mic"]
    # standardised: the restatement with the statistics' own tables (fma32: the fused multiply-add, exactly), bit for bit
    stats = ds.feature_statistics()
    ds.set_feature_statistics(stats)
    std_spec = ds.device_batch(idx, augment=rows)[0]
    ds.set_feature_statistics(None)
    scale, shift = (stats[k].numpy() for k in ("scale", "shift"))
    assert scale.dtype == np.float32 and shift.dtype == np.float32 and scale.shape == (channels, 64)
    want_std, _ = ref.gather(spec_tm, None, starts, rows, 20, ref.tetrahedron(), kind, freq_channels, MASK_VALUE, scale, shift)
    assert np.array_equal(_bits(std_spec), _bits(want_std))
    assert not np.array_equal(_bits(want_std), _bits(want_spec))
    # a pattern that is no symmetry of the array: refused before anything is launched
    bad = seld_augment.identity_rows(len(idx))
    bad[2, 0] = 5
    launched = []
    real_load = seld_native.load_library
    monkeypatch.setattr(seld_native, "load_library", lambda: (launched.append(1), real_load())[1])
    with pytest.raises(ValueError, match=r"\[5\].*no symmetries"):
        ds.device_batch(idx, augment=bad)
    assert not launched


def test_mixing_without_a_swap_on_an_array_dataset(gpu_device, class_config):
    """AUGMENT_MIX_PROB without AUGMENT_SPATIAL on an array ('logmel'): check_settings lets it through, so the feed and
    device_batch(mix=...) must run it -- the mixing pair, as on the same recordings without positions, bit for bit; any
    pattern other than 0, in a row or for a partner, is refused; GCC / NIPD features have no mix, with or without an array."""
    import seld_augment
    import trainer
    from torch.utils.data import DataLoader
    ds = _array_dataset(class_config, gpu_device, "logmel")
    plain = _array_dataset(class_config, gpu_device, "logmel", positions=None)
    assert ds.mic_array is not None and plain.mic_array is None and torch.equal(ds.spec_tm, plain.spec_tm)
    class_config.MIC_POSITIONS = "tetra_starss"
    class_config.AUGMENT_MIX_PROB = 0.6
    class_config.AUGMENT_TIME_MASKS, class_config.AUGMENT_TIME_MASK_MAX = 1, 5
    idx = list(range(len(ds)))
    rows = seld_augment.draw(3, 1, idx, class_config, window=20)
    mix = seld_augment.draw_mix(3, 1, idx, class_config, len(ds))
    assert not rows[:, 0].any() and not mix[1].any() and (mix[0] >= 0).any() and rows[:, 1:5].any()
    got_spec, got_mask = ds.device_batch(idx, augment=rows, mix=mix)
    want_spec, want_mask = plain.device_batch(idx, augment=rows, mix=mix)
    assert np.array_equal(_bits(got_spec), _bits(want_spec)) and torch.equal(got_mask, want_mask)
    unmixed = plain.device_batch(idx, augment=rows)[0]
    assert not np.array_equal(_bits(got_spec), _bits(unmixed))                  # and partners really were mixed in
    # the training feed: built without complaint, and its first batch is that of the dataset without positions
    trainer.config.SEED = 5
    try:
        feed = trainer.make_feed(DataLoader(ds, batch_size=4, shuffle=False), gpu_device, 0, 1)
        assert isinstance(feed, trainer.DeviceFeed) and feed.array is not None
        first = next(iter(feed.batches(1, augment=True)))
        class_config.MIC_POSITIONS = None
        other = next(iter(trainer.make_feed(DataLoader(plain, batch_size=4, shuffle=False), gpu_device, 0, 1)
                          .batches(1, augment=True)))
        assert np.array_equal(_bits(first[0]), _bits(other[0])) and torch.equal(first[1], other[1])
        # a Config whose positions are not the dataset's is refused when the feed is built
        with pytest.raises(ValueError, match="differs from the positions this dataset was constructed with"):
            trainer.make_feed(DataLoader(ds, batch_size=4, shuffle=False), gpu_device, 0, 1)
        class_config.MIC_POSITIONS = "tetra_starss"
        with pytest.raises(ValueError, match="differs from the positions this dataset was constructed with"):
            trainer.make_feed(DataLoader(plain, batch_size=4, shuffle=False), gpu_device, 0, 1)
        # with AUGMENT_SPATIAL beside it: refused when the feed is built, not at the first batch
        class_config.AUGMENT_SPATIAL = True
        with pytest.raises(ValueError, match="AUGMENT_MIX_PROB cannot be combined with AUGMENT_SPATIAL"):
            trainer.make_feed(DataLoader(ds, batch_size=4, shuffle=False), gpu_device, 0, 1)
        class_config.AUGMENT_SPATIAL = False
    finally:
        vars(trainer.config).pop("SEED", None)
    # patterns other than 0
    swapped = rows.copy()
    swapped[1, 0] = 9
    with pytest.raises(ValueError, match="every window's spatial pattern must be 0"):
        ds.device_batch(idx, augment=swapped, mix=mix)
    partner_swapped = (mix[0], np.where(np.arange(len(idx)) == 0, 9, mix[1]).astype(np.int32), mix[2])
    with pytest.raises(ValueError, match="every partner's spatial pattern must be 0"):
        ds.device_batch(idx, augment=rows, mix=partner_swapped)
    # GCC features: no mix is defined, at the feed and at the batch
    gcc = _array_dataset(class_config, gpu_device, "logmel_gcc")
    with pytest.raises(ValueError, match="AUGMENT_MIX_PROB is defined for power features"):
        seld_augment.check_settings(class_config, "logmel_gcc", gcc.n_channels, array=gcc.mic_array)
    with pytest.raises(ValueError, match="no mix is defined"):
        gcc.device_batch(list(range(len(gcc))), augment=seld_augment.identity_rows(len(gcc)),
                         mix=seld_augment.draw_mix(3, 1, range(len(gcc)), class_config, len(gcc)))


def test_timeline_logits_sees_the_swapped_windows(gpu_device, class_config):
    import trainer

    class Recorder(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.seen = []

        def forward(self, spec):
            self.seen.append(spec.detach().float().cpu().numpy().copy())
            return torch.zeros((spec.shape[0], 20, 648, 14), device=spec.device)

    for feature_set, kind in (("logmel_gcc", "gcc"), ("logmel_nipd", "nipd")):
        ds = _array_dataset(class_config, gpu_device, feature_set)
        model = Recorder()
        batches = list(trainer.timeline_logits(model, ds, 2, gpu_device, patterns=(0, 9, 14)))
        n = len(ds)
        assert sum(b.shape[1] for b in batches) == n and all(b.shape[0] == 3 for b in batches)
        spec_tm = ds.spec_tm.cpu().numpy()
        call = 0
        for lo in range(0, n, 2):
            idx = list(range(lo, min(lo + 2, n)))
            for p in (0, 9, 14):
                rows = np.zeros((len(idx), 12), dtype=np.int32)
                rows[:, 0] = p
                want, _ = ref.gather(spec_tm, None, ds.window_starts[idx], rows, 20, ref.tetrahedron(), kind)
                assert np.array_equal(_bits(model.seen[call]), _bits(want)), (feature_set, lo, p)
                call += 1
        assert call == len(model.seen)
        # "all" is the array's valid patterns; a pattern that is none of them is refused
        assert trainer.seld_augment.tta_patterns("all", array=ds.mic_array) == (0, 3, 4, 7, 9, 10, 13, 14)
        with pytest.raises(ValueError, match="no symmetries"):
            list(trainer.timeline_logits(model, ds, 2, gpu_device, patterns=(0, 2)))
