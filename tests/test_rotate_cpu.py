"""CPU tests of the rotation augmentation in azimuth steps: the cell permutation against the oracle's
rasteriser, the group it forms, the two float64 identities the rotating gather rests on (which pin every sign), the draw, the
refusals, the C ABI and the compiler's resource report of csrc/rotate.hip."""
import math
import re
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import augment_ref
import rotate_ref
from oracle import features as ofeat
from oracle import labels as olab

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "sound-event-localization-detection_amd" / "csrc"
I, J = 18, 36


def _cfg(**kw):
    base = dict(AUGMENT_SPATIAL=False, AUGMENT_ROTATE=False, AUGMENT_TIME_MASKS=0, AUGMENT_TIME_MASK_MAX=0, AUGMENT_FREQ_MASKS=0,
                AUGMENT_FREQ_MASK_MAX=0, AUGMENT_MASK_VALUE=0.0, FOA_CHANNEL_ORDER="WYZX", WINDOW_LENGTH=120000,
                SPECTROGRAM_HOP_LENGTH=480, GRID_CELL_DEGREES=10)
    base.update(kw)
    return SimpleNamespace(**base)


# ---------------------------------------------------------------------------------------------- 1. the cell permutation

def test_cell_dest_rot_is_a_permutation_that_extends_the_16_patterns_and_composes():
    import seld_augment
    cells = np.arange(I * J)
    seen = set()
    for m in (0, 1):
        for e in (0, 1):
            for s in range(J):
                dest, src = seld_augment.cell_dest_rot(m, s, e, I, J), seld_augment.cell_source_rot(m, s, e, I, J)
                assert np.array_equal(np.sort(dest), cells) and np.array_equal(dest[src], cells)
                moved = np.zeros(I * J, dtype=np.int64)
                moved[dest] = cells
                assert np.array_equal(moved, rotate_ref.permute_cells(cells, m, s, e, I, J))
                seen.add(dest.tobytes())
    assert len(seen) == 4 * J                                                       # 144 distinct transforms
    for p in range(16):                                                             # quarter turns: the patterns of section 11
        m, k, e = seld_augment.decode(p)
        assert np.array_equal(seld_augment.cell_dest_rot(m, k * J // 4, e, I, J), seld_augment.cell_dest(p, I, J))
        assert seld_augment.total_step(k, 0, J) == k * 9 and seld_augment.total_step(k, 31, J) == (9 * k + 31) % 36
    # the group law: (m1, s1, e1) then (m2, s2, e2) = (m1 ^ m2, s2 + (m2 ? -s1 : s1), e1 ^ e2); the same on the channels
    rng = np.random.default_rng(0)
    for _ in range(60):
        m1, m2, e1, e2 = (int(v) for v in rng.integers(0, 2, 4))
        s1, s2 = (int(v) for v in rng.integers(0, J, 2))
        first, second = seld_augment.cell_dest_rot(m1, s1, e1, I, J), seld_augment.cell_dest_rot(m2, s2, e2, I, J)
        s12 = (s2 + (-s1 if m2 else s1)) % J
        assert np.array_equal(second[first], seld_augment.cell_dest_rot(m1 ^ m2, s12, e1 ^ e2, I, J))
        x, y, z = rng.standard_normal(3)
        one = rotate_ref.field_transformed(*rotate_ref.field_transformed(x, y, z, m1, s1, e1), m2, s2, e2)
        assert np.allclose(one, rotate_ref.field_transformed(x, y, z, m1 ^ m2, s12, e1 ^ e2), atol=1e-14)
    assert np.array_equal(seld_augment.cell_dest_rot(0, 0, 0, I, J), cells)
    with pytest.raises(ValueError):
        seld_augment.total_step(1, 0, 34)


def test_rotation_table_is_double_precision_rounded_once_and_exact_at_quarter_turns():
    import seld_augment
    table = seld_augment.rotation_table(J)
    assert table.shape == (J, 2) and table.dtype == np.float32
    for k, want in enumerate(((1, 0), (0, 1), (-1, 0), (0, -1))):
        assert tuple(table[k * J // 4]) == want
    for s in range(J):
        phi = 2.0 * math.pi * s / J
        assert abs(float(table[s, 0]) - math.cos(phi)) <= 2.0 ** -24 and abs(float(table[s, 1]) - math.sin(phi)) <= 2.0 ** -24
    assert seld_augment.rotation_table(72).shape == (72, 2)
    for bad in (34, 76, 0):
        with pytest.raises(ValueError):
            seld_augment.rotation_table(bad)


def test_rotated_label_mask_equals_rasterising_the_shifted_metadata():
    """Without the mirror: every integer azimuth of [-180, 180) and every step -- a cell edge moves to a cell edge.  With the
    mirror: directions off the cell edges, where the truncating polar_to_grid commutes with it (test_augment_cpu.py)."""
    import seld_augment
    for s in range(J):
        dest = seld_augment.cell_dest_rot(0, s, 0, I, J)
        flipped = seld_augment.cell_dest_rot(0, s, 1, I, J)
        for az in range(-180, 180):
            i, j = olab.polar_to_grid(az, 37)
            az2, el2 = rotate_ref.doa(0, s, 0, az, 37)
            assert az2 == (az + 10 * s + 180) % 360 - 180
            i2, j2 = olab.polar_to_grid(az2, el2)
            assert dest[i * J + j] == i2 * J + j2, (s, az)
            i3, j3 = olab.polar_to_grid(az2, -37)
            assert flipped[i * J + j] == i3 * J + j3, (s, az)
        mirrored = seld_augment.cell_dest_rot(1, s, 0, I, J)
        for az in range(-180, 180):
            if az % 10 == 0:
                continue
            i, j = olab.polar_to_grid(az, -52)
            i2, j2 = olab.polar_to_grid(*rotate_ref.doa(1, s, 0, az, -52))
            assert mirrored[i * J + j] == i2 * J + j2, (s, az)
    # whole masks: synthetic metadata, no mirror with every row as drawn; mirror with the rows moved off the edges
    n = 24000 * 8 + 123
    rows = olab.synth_metadata(1, meta_frames=80)
    rows = rows[rows[:, 3] < 180]                                                   # azimuth 180 is -180: the wrap's own edge
    off = augment_ref.off_edge_rows(rows)
    rows[:, 4] = off[:, 4]                                                          # the FLIP needs elevations off the edges
    assert (rows[:, 3] % 10 == 0).any()                                             # azimuths stay as drawn, edges included
    mask = olab.metadata_to_mask(rows, n)
    mask_off = olab.metadata_to_mask(off, n)
    assert mask.any()
    for m, s, e in ((0, 1, 0), (0, 13, 1), (0, 35, 0), (0, 22, 1), (0, 4, 0)):
        want = olab.metadata_to_mask(rotate_ref.rows_transformed(rows, m, s, e), n)
        assert np.array_equal(mask[:, seld_augment.cell_source_rot(m, s, e, I, J)], want), (m, s, e)
        assert np.array_equal(rotate_ref.permute_cells(mask, m, s, e), want)
    for m, s, e in ((1, 1, 0), (1, 13, 1), (1, 35, 1), (1, 22, 0), (1, 4, 1), (1, 0, 0)):
        want = olab.metadata_to_mask(rotate_ref.rows_transformed(off, m, s, e), n)
        assert np.array_equal(mask_off[:, seld_augment.cell_source_rot(m, s, e, I, J)], want), (m, s, e)


# ---------------------------------------------------------------------------------------------- 2. the float64 identities

@pytest.mark.parametrize("order", ["WYZX", "WXYZ"])
def test_float64_identities_hold_on_the_plane_wave_clip(order):
    """mel |X'|^2, mel |Y'|^2 from (P_X, P_Y, C) and IV_x', IV_y' from (IV_x, IV_y), against the oracle's own features of the
    rotated clip: all 36 steps, mirror on and off, elevation flip alternating.  rtol 1e-9 on the powers, 1e-12 on the
    intensity vectors; also the share of elements that the GPU test's kappa <= 100 rule leaves out."""
    pcm = rotate_ref.plane_wave_clip(order).numpy().astype(np.float64)
    cx, cy, cz = order.index("X"), order.index("Y"), order.index("Z")
    px, py, cross = rotate_ref.rotation_terms_f64(pcm, order)
    _, mel = ofeat.logmel_f64(pcm, return_mel=True)
    assert np.allclose(mel[cx], px, rtol=1e-13) and np.allclose(mel[cy], py, rtol=1e-13)
    iv = ofeat.foa_intensity_f64(pcm)                                               # [3, 64, F]: input channels 1..3
    worst_power = worst_iv = left_out = 0.0
    for m in (0, 1):
        for s in range(J):
            e = (s + m) & 1
            phi = rotate_ref.angle(s)
            c, sn, sigma = math.cos(phi), math.sin(phi), (-1.0 if m else 1.0)
            turned = rotate_ref.pcm_transformed(pcm, m, s, e, order)
            assert np.array_equal(turned[0], pcm[0])
            _, mel_t = ofeat.logmel_f64(turned, return_mel=True)
            vx, vy = rotate_ref.combined_powers(px, py, cross, c, sn, m)
            for got, want in ((vx, mel_t[cx]), (vy, mel_t[cy])):
                assert np.allclose(got, want, rtol=1e-9, atol=0.0), (m, s)
                worst_power = max(worst_power, float(np.abs(got / want - 1.0).max()))
            assert np.array_equal(mel_t[cz], mel[cz]) and np.array_equal(mel_t[0], mel[0])
            iv_t = ofeat.foa_intensity_f64(turned)
            want_x = c * iv[cx - 1] - sn * sigma * iv[cy - 1]
            want_y = sn * iv[cx - 1] + c * sigma * iv[cy - 1]
            scale = np.abs(iv).max()
            for got, want in ((iv_t[cx - 1], want_x), (iv_t[cy - 1], want_y), (iv_t[cz - 1], -iv[cz - 1] if e else iv[cz - 1])):
                assert np.abs(got - want).max() <= 1e-12 * scale, (m, s)
                worst_iv = max(worst_iv, float(np.abs(got - want).max()))
            if s % 9:
                kx, ky = rotate_ref.cancellation(px, py, np.sqrt(px * py), c, sn, mel_t[cx], mel_t[cy])
                for kappa, v in ((kx, mel_t[cx]), (ky, mel_t[cy])):
                    db = 10.0 * np.log10(np.maximum(v, 1e-10))
                    strong = db >= db.max(axis=0, keepdims=True) - 40.0
                    left_out = max(left_out, float((kappa[strong] > 100.0).mean()))
    print(f"order {order}: worst relative power error {worst_power:.2e}, worst IV error {worst_iv:.2e}, "
          f"largest share with kappa > 100 {100 * left_out:.2f} %")
    assert np.abs(iv).max() > 0.1
    assert left_out <= 0.02


# ---------------------------------------------------------------------------------------------- 3. draw, defaults, refusals

def test_draw_is_unchanged_with_the_switch_off_and_a_function_of_seed_epoch_index_with_it_on():
    import seld_augment
    on = dict(AUGMENT_SPATIAL=True, AUGMENT_TIME_MASKS=2, AUGMENT_TIME_MASK_MAX=40, AUGMENT_FREQ_MASKS=2, AUGMENT_FREQ_MASK_MAX=12)
    # off: the generator calls of the parent commit, restated
    for kw in (on, dict(AUGMENT_SPATIAL=True), dict(AUGMENT_TIME_MASKS=1, AUGMENT_TIME_MASK_MAX=30), {}):
        got = seld_augment.draw(5, 3, np.arange(40), _cfg(**kw))
        want = np.zeros((40, 12), dtype=np.int32)
        s = seld_augment.settings(_cfg(**kw))
        for i in range(40):
            if not (s["spatial"] or s["time_masks"] or s["freq_masks"]):
                break
            rng = np.random.default_rng([5, 3, i])
            if s["spatial"]:
                want[i, 0] = rng.integers(0, 16)
            for first, count, longest, axis in ((1, s["time_masks"], s["time_max"], 250), (5, s["freq_masks"], s["freq_max"], 64)):
                for n in range(count):
                    length = int(rng.integers(0, min(longest, axis) + 1))
                    want[i, first + 2 * n] = rng.integers(0, axis - length + 1)
                    want[i, first + 2 * n + 1] = length
        assert np.array_equal(got, want) and not got[:, 9:].any()
    # on
    cfg = _cfg(AUGMENT_ROTATE=True, **{k: v for k, v in on.items() if k != "AUGMENT_SPATIAL"})
    every = seld_augment.draw(5, 1, np.arange(3000), cfg)
    assert every.shape == (3000, 12) and every.dtype == np.int32 and seld_augment.enabled(cfg)
    order = np.random.default_rng(0).permutation(3000)
    assert np.array_equal(seld_augment.draw(5, 1, order[:32], cfg), every[order[:32]])
    assert np.array_equal(seld_augment.draw(5, 1, [17, 2999, 17], cfg), every[[17, 2999, 17]])
    assert not np.array_equal(seld_augment.draw(5, 2, np.arange(3000), cfg), every)
    assert not np.array_equal(seld_augment.draw(6, 1, np.arange(3000), cfg), every)
    assert set(np.unique(every[:, 0])) == {0, 1, 8, 9}                               # m << 3 | e: k = 0
    assert every[:, 9].min() == 0 and every[:, 9].max() == J - 1 and len(np.unique(every[:, 9])) == J
    counts = np.bincount(every[:, 9], minlength=J)
    assert counts.min() > 45 and counts.max() < 125                                  # uniform: 83.3 expected, sigma 9
    assert not every[:, 10:].any() and every[:, 2].max() == 40 and every[:, 6].max() == 12
    # the switch alone, with or without AUGMENT_SPATIAL beside it: the same rows (rotation implies the spatial draw)
    alone = seld_augment.draw(5, 1, np.arange(50), _cfg(AUGMENT_ROTATE=True))
    assert np.array_equal(alone, seld_augment.draw(5, 1, np.arange(50), _cfg(AUGMENT_ROTATE=True, AUGMENT_SPATIAL=True)))
    assert alone[:, 9].any() and not alone[:, 1:9].any()
    assert seld_augment.draw(5, 1, np.arange(200), _cfg(AUGMENT_ROTATE=True), steps=72)[:, 9].max() > 36


def test_config_default_is_off_and_other_feature_sets_and_the_host_loader_are_refused():
    import seld_augment
    import trainer
    from config import Config
    assert Config.AUGMENT_ROTATE is False and not seld_augment.enabled(Config)
    assert seld_augment.settings(Config)["rotate"] is False and "AUGMENT_ROTATE" in seld_augment.SWITCHES
    seld_augment.check_settings(_cfg(AUGMENT_ROTATE=True), "logmel", 4)
    seld_augment.check_settings(_cfg(AUGMENT_ROTATE=True), "logmel_iv", 7)
    for feature_set, channels in (("logmel_gcc", 36), ("logmel", 8), ("logmel_gcc", 10)):
        with pytest.raises(ValueError, match="AUGMENT_ROTATE is defined for 4-channel FOA features"):
            seld_augment.check_settings(_cfg(AUGMENT_ROTATE=True), feature_set, channels)

    class _Windows(torch.utils.data.Dataset):
        def __len__(self):
            return 8

        def __getitem__(self, i):
            return torch.zeros(2, 4, 64), torch.zeros(2, 648, 14)

    loader = torch.utils.data.DataLoader(_Windows(), batch_size=4)
    trainer.LoaderFeed(loader, torch.device("cpu"))
    try:
        Config.AUGMENT_ROTATE = True
        with pytest.raises(RuntimeError, match="AUGMENT_ROTATE"):
            trainer.LoaderFeed(loader, torch.device("cpu"))
        with pytest.raises(RuntimeError, match="no CPU implementation"):
            trainer.make_feed(loader, torch.device("cpu"), 0, 1)
    finally:
        Config.AUGMENT_ROTATE = False
    trainer.make_feed(loader, torch.device("cpu"), 0, 1)


def test_host_parameter_table_checks_the_step_when_asked():
    import seld_native
    ok = np.zeros((2, 12), dtype=np.int32)
    ok[1, 9] = 35
    assert seld_native.augment_params(ok, 2, 250, "cpu", steps=36).dtype == torch.int32
    assert seld_native.augment_params(ok, 2, 250, "cpu")[1, 9] == 35               # the plain pair ignores the slot
    for bad in (36, -1):
        ok[1, 9] = bad
        with pytest.raises(ValueError, match="azimuth step"):
            seld_native.augment_params(ok, 2, 250, "cpu", steps=36)
    assert seld_native.foa_channels("WYZX") == (3, 1, 2) and seld_native.foa_channels("wxyz") == (1, 2, 3)
    with pytest.raises(ValueError):
        seld_native.foa_channels("XYZW")


def test_cache_file_keeps_the_rotation_terms_under_a_third_key(tmp_path):
    import dataset
    spec, mask = np.ones((5, 4, 64), np.float32), np.ones((5, 648), np.uint16)
    dataset.save_compact_features(tmp_path / "a.npz", spec, mask)
    dataset.save_compact_features(tmp_path / "b.npz", spec, mask, np.full((5, 3, 64), 2.0, np.float32))
    with np.load(tmp_path / "a.npz") as a, np.load(tmp_path / "b.npz") as b:
        assert sorted(a.files) == ["mask", "spec"] and sorted(b.files) == ["mask", "rot", "spec"]
        assert b["rot"].shape == (5, 3, 64) and np.array_equal(b["spec"], spec)


# ---------------------------------------------------------------------------------------------- 4. library and compiler

def test_library_header_and_binding_carry_the_three_entry_points():
    import seld_native
    lib = seld_native.load_library()
    header = (ROOT / "include" / "seld_hip.h").read_text()
    for name, nargs in (("seld_foa_rotation_terms", 11), ("seld_window_gather_rotate", 17), ("seld_window_permute_mask_rotate", 10)):
        assert re.search(rf"\bint {name}\(", header)
        assert len(getattr(lib, name).argtypes) == nargs
    assert "#define SELD_ROTATE_MAX_STEPS 72" in header and seld_native.AUGMENT_PARAM_INTS == 12


def test_rotate_kernels_use_no_scratch_and_no_lds_in_the_gathers():
    """Same method as test_augment_kernels_use_no_scratch: the compiler's own report for gfx950.  The label kernel of the
    rotating pair is the kStep instantiation of permute_mask_kernel in csrc/augment.hip; both instantiations are held to it."""
    import hip_resources
    found = hip_resources.report(CSRC / "rotate.hip")
    labels = {k: v for k, v in hip_resources.report(CSRC / "augment.hip").items() if "permute_mask_kernel" in k}
    assert sorted("ILb1E" in k for k in labels) == [False, True], sorted(labels)      # <false> and <true>, nothing else
    found.update(labels)
    for kernel in ("gather_rotate_kernel", "permute_mask_kernel", "rotation_terms_kernel"):
        hits = {k: v["scratch"] for k, v in found.items() if kernel in k}
        assert hits, (kernel, sorted(found))
        assert all(v == 0 for v in hits.values()), hits
    for kernel in ("gather_rotate_kernel", "permute_mask_kernel"):
        assert all(v["lds"] == 0 for k, v in found.items() if kernel in k)
