"""CPU checks of the sample-rate converter's host side (csrc/resample.hip: seld_resample_plan, seld_resample_table_host;
seld_native.resample_length) against the float64 restatement of DESIGN.md section 16.1 (tests/resample_ref.py), and of the
design itself: stop band below int16's range, pass-band ripple below the log-mel bar.  No GPU."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest

import resample_ref as ref

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "seld_hip.h"
RESPONSE_RATES = (8000, 11025, 16000, 22050, 32000, 44100, 48000, 96000, 192000)
STOP_BAND_DB = -96.3              # int16's range: 20 log10(2^-16)
RIPPLE_DB = 1e-4                  # the log-mel bar of the feature tests


@pytest.fixture(scope="module")
def native():
    import seld_native
    seld_native.load_library()
    return seld_native


@pytest.mark.parametrize("rate", ref.RATES)
def test_plan_matches_the_definition(native, rate):
    up, down, taps, half, n = ref.plan(rate)
    assert native.resample_plan(rate) == (up, down, taps, half)
    assert up <= ref.MAX_UP and taps <= ref.MAX_TAPS and taps == 2 * half + 1 and half * up >= n
    # the raw entry point, pointers that may be NULL
    lib = native.load_library()
    got = ctypes.c_int32(-1)
    assert lib.seld_resample_plan(rate, 24000, None, None, ctypes.byref(got), None) == 0 and got.value == taps


@pytest.mark.parametrize("rate,needle", [(44056, "44056"), (0, "0")])
def test_plan_rejects_what_the_design_does_not_cover(native, rate, needle):
    lib = native.load_library()
    vals = [ctypes.c_int32(-7) for _ in range(4)]
    assert lib.seld_resample_plan(rate, 24000, *[ctypes.byref(v) for v in vals]) == -1
    message = lib.seld_last_error().decode()
    assert needle in message
    if rate == 44056:
        assert "320" in message                                 # 44056 = 8 * 5507, up = 3000: the limit is named
    assert all(v.value == -7 for v in vals)                     # nothing written
    with pytest.raises(native.SeldNativeError, match=needle):
        native.resample_plan(rate)
    with pytest.raises(native.SeldNativeError):
        native.resample_length(1000, rate)
    table = np.zeros(16, dtype=np.float32)
    assert lib.seld_resample_table_host(rate, 24000, ctypes.c_void_p(table.ctypes.data), None) == -1


def test_plan_rejects_too_many_taps(native):
    lib = native.load_library()
    assert lib.seld_resample_plan(384000, 24000, None, None, None, None) == -1        # up = 1, 2155 taps
    message = lib.seld_last_error().decode()
    assert "384000" in message and "1100" in message


@pytest.mark.parametrize("rate", ref.RATES)
def test_tables_equal_the_prototype(native, rate):
    up, down, taps, half, n = ref.plan(rate)
    t32, t64 = native.resample_table(rate)
    want = ref.table_from_prototype(rate)
    assert t64.shape == want.shape == (up, taps)
    assert np.abs(t64 - want).max() <= 1e-12 * up               # a few double ulps at magnitude <= up
    assert np.array_equal(t32, t64.astype(np.float32))          # bit for bit: one rounding of the double
    assert np.array_equal(t64 == 0.0, want == 0.0)              # the zero extension past |i| <= n is exact
    assert abs(t64.sum() / up - 1.0) <= 1e-4                    # unit gain at DC
    assert np.abs(t64).sum(axis=1).max() < 2.7                  # the bound behind the GPU tests' b[m]
    # either output alone
    lib = native.load_library()
    only32 = np.zeros((up, taps), dtype=np.float32)
    assert lib.seld_resample_table_host(rate, 24000, ctypes.c_void_p(only32.ctypes.data), None) == 0
    assert np.array_equal(only32, t32)
    assert lib.seld_resample_table_host(rate, 24000, None, None) == -1


@pytest.mark.parametrize("rate", RESPONSE_RATES)
def test_frequency_response(native, rate):
    """The float64 table, re-indexed to the prototype on the dense grid fs = rate * up, through a zero-padded FFT of at
    least 16 times its length.  Gain is relative to `up` (the interpolation gain)."""
    up, down, taps, half, n = ref.plan(rate)
    _, t64 = native.resample_table(rate)
    dense = np.zeros(up * taps)
    idx = np.arange(up)[:, None] + np.arange(taps)[None, :] * up          # i + half * up
    dense[idx] = t64
    size = 1 << int(np.ceil(np.log2(16 * dense.size)))
    mag = np.abs(np.fft.rfft(dense, size)) / up
    freq = np.arange(mag.size) * (rate * up / size)
    edge = min(rate, 24000) / 2.0
    stop = 20.0 * np.log10(np.maximum(mag[freq >= edge], 1e-300)).max()
    ripple = np.abs(20.0 * np.log10(mag[freq <= 0.9 * edge])).max()
    print(f"{rate} Hz: stop band {stop:.2f} dB, pass-band ripple {ripple:.2e} dB, {taps} taps x {up} phases")
    assert stop <= STOP_BAND_DB
    assert ripple <= RIPPLE_DB


@pytest.mark.parametrize("rate", ref.RATES)
def test_resample_length(native, rate):
    up, down, *_ = ref.plan(rate)
    for length in (0, 1, down - 1, down, down + 1, 2 ** 33):
        want = -(-length * up // down)
        assert native.resample_length(length, rate) == want == ref.output_length(length, rate)


def test_header_library_and_binding_agree(native):
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    declared = set(re.findall(r"\b(seld_[a-z0-9_]+)\s*\(", text))
    lib = native.load_library()
    raw = ctypes.CDLL(str(native.LIB_PATH))
    for name in ("seld_resample_plan", "seld_resample_table_host", "seld_resample_f32", "seld_resample_i16"):
        assert name in declared
        assert hasattr(raw, name)
        assert getattr(lib, name).argtypes is not None          # declared in the binding, not only resolvable


def test_switch_defaults_off_and_cache_names_do_not_change(native, tmp_path, monkeypatch):
    import config as config_module
    import dataset
    assert config_module.Config.RESAMPLE_INPUT is False
    wav, meta = tmp_path / "a.wav", tmp_path / "a.csv"
    wav.write_bytes(b"x")
    meta.write_bytes(b"y")
    monkeypatch.setattr(dataset.config, "FEATURE_CACHE_DIR", str(tmp_path / "cache"), raising=False)
    ds = dataset.SELDDataset.__new__(dataset.SELDDataset)
    ds.use_gaussian_augmentation = False
    ds.I, ds.J, ds.sample_rate, ds.num_classes = 18, 36, 24000, 14
    off = ds._cache_path(wav, meta)
    # the name the parent commit gives: the key without a resampler token
    import hashlib
    sa, sm = wav.stat(), meta.stat()
    cfg = dataset.config
    key = "|".join(str(v) for v in (wav.resolve(), sa.st_size, sa.st_mtime_ns, meta.resolve(), sm.st_size, sm.st_mtime_ns,
                                    getattr(cfg, "FEATURE_SET", "logmel"), 18, 36, 24000, cfg.SPECTROGRAM_N_FFT,
                                    cfg.SPECTROGRAM_HOP_LENGTH, cfg.N_MELS, 14, getattr(cfg, "GRID_CELL_DEGREES", 10), "v2"))
    assert off.name == f"a.{hashlib.sha1(key.encode()).hexdigest()[:16]}.npz"
    monkeypatch.setattr(dataset.config, "RESAMPLE_INPUT", True, raising=False)
    on = ds._cache_path(wav, meta)
    assert on.name != off.name and on.parent == off.parent


def test_switch_off_still_raises_without_a_gpu_call():
    import dataset
    import torch
    assert not getattr(dataset.config, "RESAMPLE_INPUT")
    with pytest.raises(NotImplementedError, match="48000"):
        dataset.audio_to_mel_spectrogram(torch.zeros(4, 4800), 48000)
    with pytest.raises(NotImplementedError):                    # other FFT sizes still raise with the switch on
        dataset.config.RESAMPLE_INPUT = True
        try:
            dataset.audio_to_mel_spectrogram(torch.zeros(4, 4800), 48000, n_fft=1024)
        finally:
            del dataset.config.RESAMPLE_INPUT
    assert dataset.config.RESAMPLE_INPUT is False
