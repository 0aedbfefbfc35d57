"""CPU tests of the per-channel energy normalisation: the float32 restatement of the two-launch
scheme against the float64 definition (the yardstick of the GPU tests), the coefficient, the refusals on the host side,
the defaults, the ABI surface and the kernels' resources.  No GPU compute calls here."""
import ctypes
import hashlib
import math
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import hip_resources
import pcen_ref as ref

ROOT = Path(__file__).resolve().parent.parent
PKG = ROOT / "sound-event-localization-detection_amd"
HEADER = ROOT / "include" / "seld_hip.h"
NEW_SYMBOLS = ("seld_pcen", "seld_pcen_workspace")


@pytest.mark.parametrize("index", range(len(ref.SETTINGS)))
def test_ref32_error_factors(index):
    """ref32 against ref64 over every shape the GPU tests run: its error factor k in |y - y64| <= k (delta^r + |y64|) is at
    most the value recorded for the setting (the device is allowed four times that), and the recorded values are of the size
    float32 arithmetic explains: a few times 2^-23 = 1.2e-7 per operation through five transcendental steps, times the
    conditioning of 2^(x log2(10) / 10) at |x| <= 100 dB (an exponent of up to 33 rounded to float32)."""
    tau, alpha, delta, r, eps = ref.SETTINGS[index]
    s = np.float32(ref.coefficient(tau))
    worst = 0.0
    for h, (N, T, c_log, c_total) in enumerate(ref.SHAPES):
        x = ref.inputs(100 + h, N, T, c_log, c_total)
        y64 = ref.ref64(x, c_log, s, alpha, delta, r, eps)
        y32 = ref.ref32(x, c_log, s, alpha, delta, r, eps)
        assert np.isfinite(y64).all() and (y64 >= 0).all()
        k = ref.error_factor(y32, y64, delta, r)
        print(f"setting {ref.SETTINGS[index]} shape {(N, T, c_log, c_total)}: k = {k:.3e}")
        worst = max(worst, k)
    print(f"setting {ref.SETTINGS[index]}: worst k = {worst:.3e}, recorded {ref.REF32_K[index]:.1e}")
    assert worst <= ref.REF32_K[index]
    assert ref.REF32_K[index] <= 4.0e-6                      # and nothing recorded is beyond float32's reach


def test_ref64_is_the_definition():
    """A direct, scalar evaluation of the definition for one (clip, channel, bin), restart per clip included."""
    x = ref.inputs(7, 2, 40, 2, 3)
    s, alpha, delta, r, eps = np.float32(ref.coefficient(0.4)), 0.98, 2.0, 0.5, 1e-6
    y = ref.ref64(x, 2, s, alpha, delta, r, eps)
    s, alpha, eps = float(s), float(np.float32(alpha)), float(np.float32(eps))
    for n in range(2):
        e = [2.0 ** (float(v) * math.log2(10.0) / 10.0) for v in x[n, :, 1, 5]]
        m = e[0]
        for t in range(40):
            m = (1.0 - s) * m + s * e[t]
            want = (e[t] * (eps + m) ** -alpha + delta) ** r - delta ** r
            assert abs(y[n, t, 1, 5] - want) <= 1e-13 * (1.0 + abs(want))
    assert x[0, 0, 0, 0] <= -99.0 and abs(2.0 ** (-100.0 * math.log2(10.0) / 10.0) - 1e-10) < 1e-24   # the floor is 1e-10
    # the chunked float32 scheme does not depend on where the chunks are cut beyond rounding
    a = ref.ref32(x, 2, s, alpha, delta, r, eps, chunk=256)
    b = ref.ref32(x, 2, s, alpha, delta, r, eps, chunk=8)
    assert ref.error_factor(b, a, delta, r) <= 1e-6 and not np.array_equal(x[:, :, :2], a)


def test_coefficient_formula_and_limits():
    import seld_native
    for tau in (0.01, 0.06, 0.4, 2.0, 30.0):
        tf = 50.0 * tau
        want = (math.sqrt(1.0 + 4.0 * tf * tf) - 1.0) / (2.0 * tf * tf)
        assert abs(seld_native.pcen_coefficient(tau) - want) <= 1e-12 * want
        assert abs(ref.coefficient(tau) - want) <= 1e-15
        s = seld_native.pcen_coefficient(tau)
        assert abs((1.0 - s) - tf * tf * s * s) <= 1e-12          # the equation it solves: T_f^2 s^2 + s - 1 = 0
    assert abs(seld_native.pcen_coefficient(0.4) - 0.04877) < 1e-5
    for tau, *_ in ref.SETTINGS:                                  # the float the device receives is the reference's
        assert np.float32(seld_native.pcen_coefficient(tau)) == np.float32(ref.coefficient(tau))
    # tau -> 0: s -> 1 (the smoother follows the input), monotonically; tau -> infinity: s -> 1 / T_f
    values = [seld_native.pcen_coefficient(t) for t in (1e-12, 1e-6, 1e-3, 0.02, 0.4, 10.0, 1e4)]
    assert values[0] == 1.0 and abs(values[1] - 1.0) < 1e-8 and all(a > b for a, b in zip(values[1:], values[2:]))
    assert all(0.0 < v <= 1.0 for v in values)
    assert abs(values[-1] * 50.0 * 1e4 - 1.0) < 1e-5
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="time constant"):
            seld_native.pcen_coefficient(bad)


class _Cfg:
    """A Config stand-in with the switch on and everything else at its default (missing = off)."""
    PCEN = True
    PCEN_TIME_CONSTANT, PCEN_GAIN, PCEN_BIAS, PCEN_POWER, PCEN_EPS = 0.4, 0.98, 2.0, 0.5, 1e-10


def test_check_settings_refuses_what_is_defined_on_db_or_power_values():
    import seld_augment
    for name, value in (("AUGMENT_MIX_PROB", 0.5), ("AUGMENT_ROTATE", True), ("AUGMENT_LEVEL_DB", 6.0),
                        ("AUGMENT_FILTER_PROB", 0.3)):
        cfg = type("Cfg", (_Cfg,), {name: value})
        with pytest.raises(ValueError, match=rf"{name}.*PCEN"):
            seld_augment.check_settings(cfg, "logmel_iv", 7)
        off = type("Cfg", (_Cfg,), {name: value, "PCEN": False})
        seld_augment.check_settings(off, "logmel_iv", 7)                          # without PCEN the switch is fine
        with pytest.raises(ValueError, match=rf"{name}.*PCEN"):                     # ... unless the features hold PCEN values
            seld_augment.check_settings(off, "logmel_iv", 7, pcen=True)
    # what commutes with a per-channel transform stays allowed
    allowed = type("Cfg", (_Cfg,), dict(AUGMENT_SPATIAL=True, AUGMENT_TIME_MASKS=2, AUGMENT_TIME_MASK_MAX=20,
                                        AUGMENT_FREQ_MASKS=2, AUGMENT_FREQ_MASK_MAX=8, AUGMENT_CUTOUTS=2,
                                        AUGMENT_CUTOUT_TIME_MAX=10, AUGMENT_CUTOUT_FREQ_MAX=10, AUGMENT_FREQ_SHIFT_MAX=4,
                                        STANDARDISE_FEATURES=True, BALANCED_SAMPLING=True))
    seld_augment.check_settings(allowed, "logmel_iv", 7)
    seld_augment.check_settings(type("Cfg", (allowed,), {"MIC_POSITIONS": "tetra_starss"}), "logmel", 4)   # array swaps too


def test_settings_are_range_checked():
    import seld_augment
    assert seld_augment.pcen_settings(type("Cfg", (), {})) is None
    assert seld_augment.pcen_settings(_Cfg) == {"PCEN_TIME_CONSTANT": 0.4, "PCEN_GAIN": 0.98, "PCEN_BIAS": 2.0,
                                                "PCEN_POWER": 0.5, "PCEN_EPS": 1e-10}
    for name, value in (("PCEN_TIME_CONSTANT", 0.0), ("PCEN_GAIN", 1.5), ("PCEN_GAIN", -0.1), ("PCEN_BIAS", 0.0),
                        ("PCEN_POWER", 0.0), ("PCEN_POWER", 1.5), ("PCEN_EPS", 0.0), ("PCEN_EPS", float("nan"))):
        with pytest.raises(ValueError, match="PCEN"):
            seld_augment.pcen_settings(type("Cfg", (_Cfg,), {name: value}))


def test_host_loader_path_refuses_the_switch(monkeypatch):
    import trainer
    from torch.utils.data import DataLoader, TensorDataset
    loader = DataLoader(TensorDataset(torch.zeros(4, 2), torch.zeros(4, 2)), batch_size=2)
    trainer.LoaderFeed(loader, torch.device("cpu"))
    monkeypatch.setattr(type(trainer.config), "PCEN", True, raising=False)
    with pytest.raises(RuntimeError, match="PCEN"):
        trainer.LoaderFeed(loader, torch.device("cpu"))


def test_defaults_are_off_no_checkpoint_key_and_cache_names_unchanged(tmp_path, monkeypatch):
    from config import Config
    import dataset
    import trainer
    assert Config.PCEN is False
    assert (Config.PCEN_TIME_CONSTANT, Config.PCEN_GAIN, Config.PCEN_BIAS, Config.PCEN_POWER, Config.PCEN_EPS) == \
        (0.4, 0.98, 2.0, 0.5, 1e-10)
    assert trainer.PCEN_SETTINGS == ("PCEN", "PCEN_TIME_CONSTANT", "PCEN_GAIN", "PCEN_BIAS", "PCEN_POWER", "PCEN_EPS")
    # switch off: the pickled Config instance gains no attribute; on: the six names are pinned on it
    model = torch.nn.Linear(2, 2)
    opt = torch.optim.Adam(model.parameters())
    before = set(vars(trainer.config))
    payload = trainer.checkpoint_payload(1, model, opt, 0.0, 0.0)
    assert set(vars(trainer.config)) == before and not any(k.startswith("PCEN") for k in vars(payload["config"]))
    assert trainer.checkpoint_pcen_settings(payload) is None and trainer.checkpoint_pcen_settings({"epoch": 1}) is None
    monkeypatch.setattr(type(trainer.config), "PCEN", True)
    monkeypatch.setattr(type(trainer.config), "PCEN_GAIN", 0.9)
    try:
        payload = trainer.checkpoint_payload(1, model, opt, 0.0, 0.0)
        assert {k: vars(payload["config"])[k] for k in trainer.PCEN_SETTINGS} == \
            {"PCEN": True, "PCEN_TIME_CONSTANT": 0.4, "PCEN_GAIN": 0.9, "PCEN_BIAS": 2.0, "PCEN_POWER": 0.5, "PCEN_EPS": 1e-10}
        recorded = trainer.checkpoint_pcen_settings(payload)
        assert recorded == {"PCEN_TIME_CONSTANT": 0.4, "PCEN_GAIN": 0.9, "PCEN_BIAS": 2.0, "PCEN_POWER": 0.5, "PCEN_EPS": 1e-10}
    finally:
        for name in trainer.PCEN_SETTINGS:
            if name not in before and name in vars(trainer.config):
                delattr(trainer.config, name)
    monkeypatch.undo()

    # evaluation names both sides when dataset and checkpoint disagree
    built_off, built_on = type("D", (), {"pcen_settings": None})(), type("D", (), {"pcen_settings": dict(recorded)})()
    trainer.check_dataset_pcen(None, built_off, "the checkpoint records")
    trainer.check_dataset_pcen(recorded, built_on, "the checkpoint records")
    with pytest.raises(ValueError, match=r"built with PCEN off, the checkpoint records with PCEN on with .*PCEN_GAIN = 0.9"):
        trainer.check_dataset_pcen(recorded, built_off, "the checkpoint records")
    with pytest.raises(ValueError, match=r"built with PCEN on with .*, the checkpoint records with PCEN off"):
        trainer.check_dataset_pcen(None, built_on, "the checkpoint records")
    with pytest.raises(ValueError, match="PCEN_GAIN = 0.98"):
        trainer.check_dataset_pcen(dict(recorded, PCEN_GAIN=0.98), built_on, "the checkpoint records")

    # cache names: what the parent commit gives with the switch off; another name per setting with it on
    wav, meta = tmp_path / "a.wav", tmp_path / "a.csv"
    wav.write_bytes(b"x")
    meta.write_bytes(b"y")
    monkeypatch.setattr(dataset.config, "FEATURE_CACHE_DIR", str(tmp_path / "cache"), raising=False)
    ds = dataset.SELDDataset.__new__(dataset.SELDDataset)
    ds.use_gaussian_augmentation = False
    ds.I, ds.J, ds.sample_rate, ds.num_classes = 18, 36, 24000, 14
    ds.pcen_settings = None
    sa, sm = wav.stat(), meta.stat()
    cfg = dataset.config
    key = "|".join(str(v) for v in (wav.resolve(), sa.st_size, sa.st_mtime_ns, meta.resolve(), sm.st_size, sm.st_mtime_ns,
                                    getattr(cfg, "FEATURE_SET", "logmel"), 18, 36, 24000, cfg.SPECTROGRAM_N_FFT,
                                    cfg.SPECTROGRAM_HOP_LENGTH, cfg.N_MELS, 14, getattr(cfg, "GRID_CELL_DEGREES", 10), "v2"))
    off = ds._cache_path(wav, meta)
    assert off.name == f"a.{hashlib.sha1(key.encode()).hexdigest()[:16]}.npz"
    ds.pcen_settings = dict(recorded)
    on = ds._cache_path(wav, meta)
    ds.pcen_settings = dict(recorded, PCEN_EPS=1e-6)
    other = ds._cache_path(wav, meta)
    assert len({off.name, on.name, other.name}) == 3 and on.parent == off.parent


def test_new_symbols_are_declared_exported_and_bound():
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    declared = set(re.findall(r"\b(seld_[a-z0-9_]+)\s*\(", text))
    assert {n for n in declared if "pcen" in n} == set(NEW_SYMBOLS)
    assert re.search(r"#define\s+SELD_PCEN_CHUNK_FRAMES\s+256\b", HEADER.read_text())
    lib_path = PKG / "libseld_hip.so"
    if not lib_path.exists():
        import __graft_entry__
        __graft_entry__.build()
    raw = ctypes.CDLL(str(lib_path))
    import seld_native
    lib = seld_native.load_library()
    for name in NEW_SYMBOLS:
        assert hasattr(raw, name), name
        assert getattr(lib, name).argtypes is not None, name
    assert seld_native.PCEN_CHUNK_FRAMES == ref.CHUNK == 256
    assert callable(seld_native.pcen) and callable(seld_native.pcen_coefficient)
    # the workspace size is host arithmetic: float [N][chunks][C_log][64]; 0 for refused extents
    size = lib.seld_pcen_workspace
    assert size(1, 1, 4, 4) == 1 * 1 * 4 * 256 and size(3, 257, 7, 4) == 3 * 2 * 4 * 256
    assert size(2, 1300, 36, 8) == 2 * 6 * 8 * 256 and size(1, 180000, 7, 4) == 704 * 4 * 256
    for bad in ((0, 10, 4, 4), (1, 0, 4, 4), (1, 10, 4, 0), (1, 10, 4, 5), (1, 1 << 31, 4, 4), (1 << 40, 1000, 4, 4)):
        assert size(*bad) == 0, bad
    # an uninitialised process is told so before any argument is looked at (this process never calls seld_init)
    if not torch.cuda.is_available():
        assert lib.seld_pcen(None, None, 0, 0, 0, 0, 0.0, 0.0, 0.0, 0.0, 0.0, None, 0, None) == -3


def test_kernels_use_no_scratch_and_no_lds():
    """The compiler's resource report: the two kernels of csrc/pcen.hip report zero scratch and zero LDS (DESIGN.md section
    30.2 states none), and their registers leave at least four waves per SIMD."""
    report = hip_resources.report(PKG / "csrc" / "pcen.hip")
    for kernel in ("pcen_carry_kernel", "pcen_apply_kernel"):
        hits = {k: v for k, v in report.items() if kernel in k}
        assert len(hits) == 1, (kernel, sorted(report))
        row = next(iter(hits.values()))
        print(kernel, row)
        assert row["scratch"] == 0 and row["lds"] == 0, (kernel, row)
        assert row["vgprs"] <= 128 and row["occupancy"] >= 4, (kernel, row)
    assert len(report) == 2, sorted(report)
