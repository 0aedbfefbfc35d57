"""CPU tests of the per-bin feature standardisation: the restated summation order against math.fsum,
seld_standardise.finalise and its edge cases, the checkpoint payload round trip, the Config default, the compiler's resource
report of the new kernels, and the declared symbols."""
import ctypes
import math
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import hip_resources
import seld_standardise
import standardise_ref as ref

ROOT = Path(__file__).resolve().parent.parent
PKG = ROOT / "sound-event-localization-detection_amd"
CSRC = PKG / "csrc"
HEADER = ROOT / "include" / "seld_hip.h"
NEW_SYMBOLS = ("seld_feature_moments", "seld_feature_moments_workspace", "seld_window_gather_affine",
               "seld_window_gather_augment_affine", "seld_window_gather_rotate_affine")


_features = ref.feature_like


def test_restated_moments_agree_with_fsum():
    """The slab order of tests/standardise_ref.py (what the kernel is held to, bit for bit, on the GPU) against the exactly
    rounded sum of every column: 1e-12 relative.  2100 frames at slab 1024: two full slabs and a ragged one."""
    x = np.ascontiguousarray(_features(1, 2100, 3)[:, :, :8])
    got = ref.moments(x)
    for c in range(3):
        for f in range(8):
            col = x[:, c, f].astype(np.float64)
            s1, s2 = math.fsum(col), math.fsum(col * col)
            assert abs(got[0, c, f] - s1) <= 1e-12 * abs(s1), (c, f)
            assert abs(got[1, c, f] - s2) <= 1e-12 * s2, (c, f)
    # the order is part of the definition: one slab over everything is another (equally good) sum, and the ragged last
    # slab is a slab of its own
    assert np.array_equal(ref.moments(x[:1024]), ref.moments(x[:1024], slab=4096))
    assert got.shape == (2, 3, 8) and got.dtype == np.float64
    assert ref.FLAT_STD == seld_standardise.FLAT_STD and ref.SLAB == 1024


def test_finalise_matches_the_restatement_and_its_edge_cases():
    x = _features(2, 300, 4)
    m = ref.moments(x)
    stats = seld_standardise.finalise(torch.from_numpy(m), 300)
    mean, std, scale, shift = ref.finalise(m, 300)
    assert np.array_equal(stats["mean"].numpy(), mean) and np.array_equal(stats["std"].numpy(), std)
    assert stats["scale"].dtype == torch.float32 and stats["shift"].dtype == torch.float32
    assert np.array_equal(stats["scale"].numpy().view(np.uint32), scale.view(np.uint32))
    assert np.array_equal(stats["shift"].numpy().view(np.uint32), shift.view(np.uint32))
    assert stats["frames"] == 300 and all(t.device.type == "cpu" for t in stats.values() if isinstance(t, torch.Tensor))
    assert np.allclose(stats["mean"].numpy(), x.astype(np.float64).mean(axis=0), rtol=0, atol=1e-9)
    assert np.allclose(stats["std"].numpy(), x.astype(np.float64).std(axis=0), rtol=1e-9, atol=1e-9)

    # a flat bin is only centred: scale 1, shift -mean
    flat = x.copy()
    flat[:, 1, 5] = -100.0
    s = seld_standardise.finalise(ref.moments(flat), 300)
    assert s["std"][1, 5] == 0.0 and s["scale"][1, 5] == 1.0 and s["shift"][1, 5] == 100.0
    assert s["scale"][1, 6] == np.float32(1.0 / float(s["std"][1, 6]))

    # T = 1: every bin is flat
    one = seld_standardise.finalise(ref.moments(x[:1]), 1)
    assert bool((one["std"] == 0).all()) and bool((one["scale"] == 1).all())
    assert np.array_equal(one["shift"].numpy(), (-x[0].astype(np.float64)).astype(np.float32))

    # negative round-off in the variance: S2 / T - mean^2 < 0 for a constant that is not a dyadic rational
    v = np.float32(0.1)
    m2 = np.zeros((2, 1, 64))
    m2[0], m2[1] = 3 * float(v), 3 * float(v) * float(v) * (1 - 1e-13)
    assert (m2[1] / 3 - (m2[0] / 3) ** 2 < 0).all()
    neg = seld_standardise.finalise(m2, 3)
    assert bool((neg["std"] == 0).all()) and bool((neg["scale"] == 1).all()) and bool(torch.isfinite(neg["shift"]).all())

    # non-finite moments are refused, as are nonsense frame counts and shapes
    for bad in (float("nan"), float("inf")):
        m3 = m.copy()
        m3[1, 2, 3] = bad
        with pytest.raises(ValueError, match="non-finite"):
            seld_standardise.finalise(m3, 300)
    with pytest.raises(ValueError):
        seld_standardise.finalise(m, 0)
    with pytest.raises(ValueError):
        seld_standardise.finalise(m[0], 300)


def test_payload_round_trip_is_exact(tmp_path):
    stats = seld_standardise.finalise(ref.moments(_features(3, 200, 7)), 200)
    payload = seld_standardise.to_payload(stats, "logmel_iv", 7)
    assert sorted(payload) == sorted(("mean", "std", "frames", "feature_set", "channels"))
    assert payload["mean"].dtype == torch.float64 and payload["mean"].device.type == "cpu"
    assert payload["mean"] is not stats["mean"]                      # a copy, never the live tensors
    torch.save({"feature_statistics": payload}, tmp_path / "ckpt.pth")
    loaded = torch.load(tmp_path / "ckpt.pth", weights_only=True)["feature_statistics"]
    back = seld_standardise.from_payload(loaded, channels=7, feature_set="logmel_iv")
    for key in ("mean", "std", "scale", "shift"):
        assert back[key].dtype == stats[key].dtype
        assert torch.equal(back[key].view(torch.int64 if back[key].dtype == torch.float64 else torch.int32),
                           stats[key].view(torch.int64 if stats[key].dtype == torch.float64 else torch.int32)), key
    assert back["frames"] == 200
    with pytest.raises(ValueError, match="channels"):
        seld_standardise.from_payload(loaded, channels=4)
    with pytest.raises(ValueError, match="FEATURE_SET"):
        seld_standardise.from_payload(loaded, feature_set="logmel")
    with pytest.raises(KeyError):
        seld_standardise.from_payload({k: v for k, v in loaded.items() if k != "std"})

    # the checkpoint decides; switch on and no statistics: an error of the EVAL_USE_EMA shape
    class Cfg:
        STANDARDISE_FEATURES = False
    assert seld_standardise.checkpoint_statistics({"epoch": 1}, Cfg) is None
    assert seld_standardise.checkpoint_statistics({"feature_statistics": loaded}, Cfg, channels=7)["frames"] == 200
    Cfg.STANDARDISE_FEATURES = True
    with pytest.raises(KeyError, match="feature_statistics"):
        seld_standardise.checkpoint_statistics({"epoch": 1}, Cfg)


def test_config_default_is_off_and_checkpoints_carry_no_new_key():
    from config import Config
    assert Config.STANDARDISE_FEATURES is False
    import trainer
    assert trainer.standardise_datasets(object(), object()) is None          # off: nothing is looked at
    model = torch.nn.Linear(2, 2)
    opt = torch.optim.Adam(model.parameters())
    assert "feature_statistics" not in trainer.checkpoint_payload(1, model, opt, 0.0, 0.0)
    assert trainer.checkpoint_payload(1, model, opt, 0.0, 0.0, {"frames": 3})["feature_statistics"] == {"frames": 3}


def test_host_loader_path_refuses_the_switch(monkeypatch):
    import trainer
    from torch.utils.data import DataLoader, TensorDataset
    loader = DataLoader(TensorDataset(torch.zeros(4, 2), torch.zeros(4, 2)), batch_size=2)
    trainer.LoaderFeed(loader, torch.device("cpu"))
    monkeypatch.setattr(type(trainer.config), "STANDARDISE_FEATURES", True, raising=False)
    with pytest.raises(RuntimeError, match="STANDARDISE_FEATURES"):
        trainer.LoaderFeed(loader, torch.device("cpu"))


def test_new_kernels_use_no_scratch_and_no_lds():
    """The compiler's resource report (the recipe of test_hot_kernels_do_not_spill): the moments kernels and BOTH
    instantiations of the three gathers report zero scratch and zero LDS; the standardising instantiations exist."""
    wanted = {"standardise.hip": ("moment_slab_kernel", "moment_fold_kernel"),
              "labels.hip": ("gather_rows_kernelILb0", "gather_rows_kernelILb1"),
              "augment.hip": ("gather_augment_kernelILb0", "gather_augment_kernelILb1"),
              "rotate.hip": ("gather_rotate_kernelILb0", "gather_rotate_kernelILb1")}
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(max_workers=4) as pool:
        reports = dict(zip(wanted, pool.map(lambda name: hip_resources.report(CSRC / name), wanted)))
    for name, kernels in wanted.items():
        for kernel in kernels:
            hits = {k: v for k, v in reports[name].items() if kernel in k}
            assert len(hits) == 1, (name, kernel, sorted(reports[name]))
            row = next(iter(hits.values()))
            print(name, kernel, row)
            assert row["scratch"] == 0 and row["lds"] == 0, (name, kernel, row)


def test_new_symbols_are_declared_exported_and_bound():
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    declared = set(re.findall(r"\b(seld_[a-z0-9_]+)\s*\(", text))
    added = {n for n in declared if "affine" in n or "moments" in n}
    assert added == set(NEW_SYMBOLS)
    assert re.search(r"#define\s+SELD_MOMENT_SLAB_FRAMES\s+1024\b", HEADER.read_text())
    assert ref.SLAB == 1024
    lib_path = PKG / "libseld_hip.so"
    if not lib_path.exists():
        import __graft_entry__
        __graft_entry__.build()
    raw = ctypes.CDLL(str(lib_path))
    import seld_native
    lib = seld_native.load_library()
    for name in NEW_SYMBOLS:
        assert hasattr(raw, name), name
        assert getattr(lib, name).argtypes is not None, f"{name}: no ctypes declaration in seld_native"
    assert lib.seld_feature_moments_workspace.restype is ctypes.c_int64
    # the workspace: one [2][C][64] double block per slab; refused extents report 0
    assert lib.seld_feature_moments_workspace(1, 4) == 2 * 4 * 64 * 8
    assert lib.seld_feature_moments_workspace(1024, 7) == 2 * 7 * 64 * 8
    assert lib.seld_feature_moments_workspace(1025, 7) == 2 * 2 * 7 * 64 * 8
    assert lib.seld_feature_moments_workspace(0, 7) == 0 and lib.seld_feature_moments_workspace(5, 0) == 0
    for fn in ("feature_moments", "gather_windows_affine"):
        assert callable(getattr(seld_native, fn))
    # without a GPU there is no fallback, and no device is "library not initialised": -3 before any argument is looked at
    if not torch.cuda.is_available():
        assert lib.seld_feature_moments(None, 0, 0, None, None, 0, None) == -3
    with pytest.raises(seld_native.SeldNativeError):
        seld_native.feature_moments(torch.zeros(8, 4, 64))
