"""CPU tests of the channel swap for microphone arrays (seld_augment.py, csrc/micswap.hip): which
patterns are symmetries of which array and with which permutation, the physics behind "channel j of the transformed scene
is channel sigma(j) of the recording", the draw, every refusal of the host side, and the kernels' resources."""
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

import hip_resources
import mic_swap_ref as ref
import seld_augment as aug

ROOT = Path(__file__).resolve().parent.parent
SQUARE = [(0.03, 0.03, 0.0), (-0.03, 0.03, 0.0), (-0.03, -0.03, 0.0), (0.03, -0.03, 0.0)]
LINE = [(-0.06, 0.0, 0.0), (-0.02, 0.0, 0.0), (0.02, 0.0, 0.0), (0.06, 0.0, 0.0)]
IRREGULAR = [(0.031, 0.012, 0.004), (-0.027, 0.035, -0.011), (0.005, -0.041, 0.019), (-0.013, -0.008, -0.037)]
GEOMETRIES = {"tetra": (ref.tetrahedron(), [0, 3, 4, 7, 9, 10, 13, 14]), "cube": (ref.cube(), list(range(16))),
              "square": (SQUARE, list(range(16))), "line": (LINE, [0, 1, 4, 5, 8, 9, 12, 13]), "irregular": (IRREGULAR, [0])}


def _cfg(**over):
    base = dict(AUGMENT_SPATIAL=False, AUGMENT_ROTATE=False, AUGMENT_TIME_MASKS=0, AUGMENT_TIME_MASK_MAX=0, AUGMENT_FREQ_MASKS=0,
                AUGMENT_FREQ_MASK_MAX=0, AUGMENT_MASK_VALUE=0.0, FOA_CHANNEL_ORDER="WYZX", AUGMENT_MIX_PROB=0.0,
                AUGMENT_MIX_GAIN_DB=6.0, GRID_CELL_DEGREES=10, WINDOW_LENGTH=24000, SPECTROGRAM_HOP_LENGTH=480, MIC_POSITIONS=None)
    base.update(over)
    return SimpleNamespace(**base)


@pytest.mark.parametrize("name", sorted(GEOMETRIES))
def test_valid_patterns_of_the_five_geometries(name):
    positions, valid = GEOMETRIES[name]
    assert list(aug.mic_valid_patterns(positions)) == valid
    assert ref.valid_patterns(positions) == valid
    table = aug.mic_permutations(positions)
    assert table.dtype == np.int8 and table.shape == (16, len(positions))
    for p in range(16):
        want = ref.sigma(positions, p)
        assert table[p].tolist() == (want if want is not None else [-1] * len(positions))
    assert table[0].tolist() == list(range(len(positions)))


def test_tetrahedron_preset_and_its_table():
    pos = aug.mic_positions("tetra_starss")
    assert pos.dtype == np.float64 and pos.shape == (4, 3)
    assert np.abs(pos - ref.tetrahedron()).max() <= 1e-15
    assert np.abs(np.linalg.norm(pos, axis=1) - 0.042).max() <= 1e-15
    table = aug.mic_permutations("tetra_starss")
    assert {p: table[p].tolist() for p in range(16) if table[p, 0] >= 0} == ref.TETRA_SIGMA
    assert ref.TETRA_SIGMA == {0: [0, 1, 2, 3], 3: [1, 3, 0, 2], 4: [3, 2, 1, 0], 7: [2, 0, 3, 1], 9: [1, 0, 3, 2],
                               10: [0, 2, 1, 3], 13: [2, 3, 0, 1], 14: [3, 1, 2, 0]}


def test_square_flips_keep_every_microphone():
    table = aug.mic_permutations(SQUARE)
    for p in range(0, 16, 2):
        assert table[p + 1].tolist() == table[p].tolist()          # the flip z -> -z moves nothing in the z = 0 plane
    assert table[1].tolist() == [0, 1, 2, 3]


def test_logmel_channel_table_is_sigma():
    table = aug.mic_channel_table("tetra_starss")
    assert table.dtype == np.uint8 and table.shape == (16, 4)
    for p in range(16):
        assert table[p].tolist() == ref.TETRA_SIGMA.get(p, [0, 1, 2, 3])


@pytest.mark.parametrize("name", ["tetra", "cube"])
def test_path_lengths_of_a_moved_source(name):
    """r_j . (T_p d) == r_sigma(j) . d: the source at T_p d reaches microphone j as the source at d reaches sigma(j)."""
    positions, valid = GEOMETRIES[name]
    positions = np.asarray(positions)
    d = np.random.default_rng(3).normal(size=(20, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    for p in valid:
        sig = aug.mic_permutations(positions)[p]
        assert np.abs(aug.pattern_matrix(p) @ d[0] - ref.apply_pattern(p, d[0])).max() <= 1e-15
        assert np.abs(positions @ ref.apply_pattern(p, d).T - positions[sig] @ d.T).max() <= 1e-12


@pytest.mark.parametrize("name", ["tetra", "cube"])
def test_ideal_nipd_follows_the_rule(name):
    """c (tau_i - tau_0) of a plane wave from T_p d at the array = the NIPD rule N(sigma(m)) - N(sigma(0)) on the ideal NIPD
    of the plane wave from d (float64, no wrapping: the rule is exact).  sigma is the host code's (mic_permutations), the
    rule the restatement's (transform_rows, what the GPU tests hold the kernel to): a wrong convention in either fails."""
    positions, valid = GEOMETRIES[name]
    positions = np.asarray(positions)
    C = len(positions)
    d = np.random.default_rng(4).normal(size=(20, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    path = lambda dirs: -(positions @ dirs.T)                      # c tau_j: a microphone towards the source hears it early
    nipd = lambda dirs: (path(dirs)[1:] - path(dirs)[:1]).T        # [20, C-1], reference microphone 0

    def feature_rows(dirs):
        """float64 [20, 2C - 1, 64]: channel c < C holds the microphone's own path length, then the ideal NIPD channels."""
        rows = np.concatenate([path(dirs).T, nipd(dirs)], axis=1)
        return np.repeat(rows[:, :, None], 64, axis=2)

    table = aug.mic_permutations(positions)
    for p in valid:
        sig = table[p].tolist()
        ruled = ref.transform_rows(feature_rows(d), sig, "nipd")
        assert ruled.dtype == np.float64
        assert np.abs(ruled - feature_rows(ref.apply_pattern(p, d))).max() <= 1e-12
    moved = [p for p in valid if table[p, 0] != 0]
    assert moved                                                    # the difference form is exercised, not only copies


def test_draw_without_positions_is_todays_draw():
    """MIC_POSITIONS None: the rows of FOA settings are what the generator gave before arrays existed (restated here)."""
    cfg = _cfg(AUGMENT_SPATIAL=True, AUGMENT_TIME_MASKS=2, AUGMENT_TIME_MASK_MAX=9, AUGMENT_FREQ_MASKS=1, AUGMENT_FREQ_MASK_MAX=7)
    bare = _cfg(AUGMENT_SPATIAL=True, AUGMENT_TIME_MASKS=2, AUGMENT_TIME_MASK_MAX=9, AUGMENT_FREQ_MASKS=1, AUGMENT_FREQ_MASK_MAX=7)
    del bare.MIC_POSITIONS                                          # a Config from before the attribute existed
    idx = np.arange(40)
    rows = aug.draw(11, 3, idx, cfg, window=50)
    assert np.array_equal(rows, aug.draw(11, 3, idx, bare, window=50))
    want = np.zeros_like(rows)
    for r, i in enumerate(idx):
        rng = np.random.default_rng([11, 3, int(i)])
        want[r, 0] = rng.integers(0, 16)
        for first, count, longest, axis in ((1, 2, 9, 50), (5, 1, 7, 64)):
            for n in range(count):
                length = int(rng.integers(0, min(longest, axis) + 1))
                want[r, first + 2 * n] = rng.integers(0, axis - length + 1)
                want[r, first + 2 * n + 1] = length
    assert np.array_equal(rows, want)
    assert len(set(rows[:, 0].tolist())) > 8                        # over all 16, not over some array's


def test_draw_on_an_array():
    cfg = _cfg(AUGMENT_SPATIAL=True, AUGMENT_TIME_MASKS=1, AUGMENT_TIME_MASK_MAX=5, MIC_POSITIONS="tetra_starss")
    valid = [0, 3, 4, 7, 9, 10, 13, 14]
    rows = aug.draw(5, 2, np.arange(400), cfg, window=50)
    assert set(rows[:, 0].tolist()) == set(valid)                  # valid patterns only, every one of them within 400 windows
    for r, i in enumerate(range(400)):                             # valid[rng.integers(0, len(valid))], then the masks
        rng = np.random.default_rng([5, 2, i])
        assert rows[r, 0] == valid[int(rng.integers(0, 8))]
    # a row is a function of (seed, epoch, window index) only: not of the batch, its order or its size
    picked = np.array([399, 7, 7, 120])
    assert np.array_equal(aug.draw(5, 2, picked, cfg, window=50), rows[picked])
    assert not np.array_equal(aug.draw(5, 3, np.arange(400), cfg, window=50)[:, 0], rows[:, 0])
    assert not np.array_equal(aug.draw(6, 2, np.arange(400), cfg, window=50)[:, 0], rows[:, 0])
    # without AUGMENT_SPATIAL the array changes nothing: identity patterns, the same masks as without positions
    off = _cfg(AUGMENT_TIME_MASKS=1, AUGMENT_TIME_MASK_MAX=5, MIC_POSITIONS="tetra_starss")
    assert np.array_equal(aug.draw(5, 2, np.arange(30), off, window=50),
                          aug.draw(5, 2, np.arange(30), _cfg(AUGMENT_TIME_MASKS=1, AUGMENT_TIME_MASK_MAX=5), window=50))


def test_mic_positions_refusals():
    assert aug.mic_positions(None) is None
    got = aug.mic_positions(SQUARE)
    assert got.dtype == np.float64 and got.shape == (4, 3)
    for bad in ("tetra", [(0.0, 0.0, 0.1)], [], [(0.1, 0.0), (0.2, 0.0)], [(0.1, 0.0, 0.0), (np.nan, 0.0, 0.0)],
                [(0.1, 0.0, 0.0), (np.inf, 0.0, 0.0)], [(0.1, 0.0, 0.0), (0.1, 0.0, 0.0)], [(0.1, 0.0, 0.0), "x"]):
        with pytest.raises(ValueError):
            aug.mic_positions(bad)


def test_check_settings_with_an_array():
    tetra = aug.mic_positions("tetra_starss")
    on = _cfg(AUGMENT_SPATIAL=True)
    # without an array: today's refusal, word for word
    with pytest.raises(ValueError, match="a microphone array's geometry is unknown here, so no channel swap is defined"):
        aug.check_settings(on, "logmel_gcc", 10)
    for feature_set, channels in (("logmel", 4), ("logmel_gcc", 10), ("logmel_nipd", 7)):
        aug.check_settings(on, feature_set, channels, array=tetra)
        aug.check_settings(_cfg(AUGMENT_SPATIAL=True, MIC_POSITIONS="tetra_starss"), feature_set, channels)
    aug.check_settings(on, "logmel_gcc", 36, array=ref.cube())
    aug.check_settings(on, "logmel_nipd", 15, array=ref.cube())
    with pytest.raises(ValueError, match="logmel_iv"):
        aug.check_settings(on, "logmel_iv", 7, array=tetra)
    with pytest.raises(ValueError, match="AUGMENT_ROTATE"):
        aug.check_settings(_cfg(AUGMENT_ROTATE=True), "logmel", 4, array=tetra)
    with pytest.raises(ValueError, match="AUGMENT_MIX_PROB"):
        aug.check_settings(_cfg(AUGMENT_SPATIAL=True, AUGMENT_MIX_PROB=0.5), "logmel", 4, array=tetra)
    aug.check_settings(_cfg(AUGMENT_MIX_PROB=0.5), "logmel", 4, array=tetra)       # mixing alone stays what it was
    for feature_set, channels in (("logmel", 8), ("logmel_gcc", 36), ("logmel_nipd", 15), ("logmel_gcc", 11), ("logmel_nipd", 8)):
        with pytest.raises(ValueError, match="4 microphones"):
            aug.check_settings(on, feature_set, channels, array=tetra)


def test_check_tta_with_an_array():
    tetra = aug.mic_positions("tetra_starss")
    with pytest.raises(ValueError, match="a microphone array's geometry is unknown here, so no channel swap is defined"):
        aug.check_tta((0, 9), "logmel_nipd", 7)
    aug.check_tta((0, 9, 14), "logmel_nipd", 7, array=tetra)
    aug.check_tta((), "logmel_iv", 7, array=tetra)                  # off: nothing to refuse
    with pytest.raises(ValueError, match=r"\[1, 2\].*\[0, 3, 4, 7, 9, 10, 13, 14\]"):
        aug.check_tta((0, 1, 2, 9), "logmel_gcc", 10, array=tetra)
    with pytest.raises(ValueError, match="logmel_iv"):
        aug.check_tta((0,), "logmel_iv", 7, array=tetra)
    with pytest.raises(ValueError, match="4 microphones"):
        aug.check_tta((0,), "logmel_gcc", 36, array=tetra)
    assert aug.tta_patterns("all") == tuple(range(16))
    assert aug.tta_patterns("all", array=tetra) == (0, 3, 4, 7, 9, 10, 13, 14)
    assert aug.tta_patterns("0,9", array=tetra) == (0, 9)


def test_config_default_is_off():
    from config import Config
    assert Config.MIC_POSITIONS is None


def test_kernels_use_no_scratch_and_no_lds():
    found = hip_resources.report(ROOT / "sound-event-localization-detection_amd" / "csrc" / "micswap.hip")
    kernels = {k: v for k, v in found.items() if "gather_mic_kernel" in k}
    assert len(kernels) == 2, sorted(found)
    for name, row in found.items():
        assert row["scratch"] == 0 and row["lds"] == 0, (name, row)
