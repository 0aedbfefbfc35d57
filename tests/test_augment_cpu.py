"""CPU tests of the training augmentation: the host tables against the oracle's rasteriser, the group
structure of the 16 patterns, the per-window draw, the compiler's resource report of the two kernels, the host-path error."""
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import augment_ref
from oracle import labels as olab

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "sound-event-localization-detection_amd" / "csrc"
I, J = 18, 36


def _cfg(**kw):
    base = dict(AUGMENT_SPATIAL=False, AUGMENT_TIME_MASKS=0, AUGMENT_TIME_MASK_MAX=0, AUGMENT_FREQ_MASKS=0,
                AUGMENT_FREQ_MASK_MAX=0, AUGMENT_MASK_VALUE=0.0, FOA_CHANNEL_ORDER="WYZX", WINDOW_LENGTH=120000,
                SPECTROGRAM_HOP_LENGTH=480)
    base.update(kw)
    return SimpleNamespace(**base)


# ---------------------------------------------------------------------------------------------- 1. labels vs the rasteriser

@pytest.mark.parametrize("clip", [0, 1, 2])
def test_label_permutation_equals_rasterising_the_transformed_metadata(clip):
    """Every one of the 16 patterns: permuting the cells of metadata_to_mask(rows) is bit-equal to rasterising the rows with
    (az', el').  The DOAs are drawn as synth_metadata draws them and moved off the cell edges (augment_ref.off_edge_rows),
    where the reference's truncating polar_to_grid commutes with the mirror; no pattern and no row is left out."""
    import seld_augment
    rows = augment_ref.off_edge_rows(olab.synth_metadata(clip, meta_frames=80))
    assert not (rows[:, 3] % 10 == 0).any() and not (rows[:, 4] % 10 == 0).any()
    n = 24000 * 8 + 123
    mask = olab.metadata_to_mask(rows, n)
    assert mask.any()
    for p in range(16):
        want = olab.metadata_to_mask(augment_ref.rows_transformed(rows, p), n)
        assert np.array_equal(augment_ref.permute_cells(mask, p), want), p
        assert np.array_equal(mask[:, seld_augment.cell_source(p, I, J)], want), p        # the host table, gather form
        moved = np.zeros_like(mask)
        moved[:, seld_augment.cell_dest(p, I, J)] = mask                                  # and its scatter form
        assert np.array_equal(moved, want), p


def test_every_integer_direction_off_the_cell_edges_commutes():
    """polar_to_grid computes i from the elevation and j from the azimuth independently, so checking every integer azimuth
    and every integer elevation off the edges under all 16 patterns covers all 65 341 integer directions."""
    import seld_augment
    checked = 0
    for p in range(16):
        dest = seld_augment.cell_dest(p, I, J)
        for az in range(-180, 181):
            if az % 10 == 0:
                continue
            i, j = olab.polar_to_grid(az, 37)
            az2, el2 = augment_ref.doa(p, az, 37)
            i2, j2 = olab.polar_to_grid(az2, el2)
            assert dest[i * J + j] == i2 * J + j2, (p, az)
            checked += 1
        for el in range(-90, 91):
            if el % 10 == 0:
                continue
            i, j = olab.polar_to_grid(-123, el)
            az2, el2 = augment_ref.doa(p, -123, el)
            i2, j2 = olab.polar_to_grid(az2, el2)
            assert dest[i * J + j] == i2 * J + j2, (p, el)
            checked += 1
    assert checked == 16 * (324 + 162)
    # and why the definition is on cells: on an edge the truncation does not commute with the mirror
    assert olab.polar_to_grid(-10, 5)[1] == 17 and olab.polar_to_grid(10, 5)[1] == 19 and J - 1 - 19 == 16


# ---------------------------------------------------------------------------------------------- 2. group structure

def _signed_matrix(row):
    """The intensity-vector part of a 7-channel table row as a signed 3 x 3 permutation matrix: new = M @ old."""
    m = np.zeros((3, 3), dtype=int)
    for c in range(3):
        m[c, (int(row[4 + c]) & 0x7f) - 4] = -1 if row[4 + c] & 0x80 else 1
    return m


def test_patterns_form_a_group_of_signed_permutations():
    import seld_augment
    cells = np.arange(I * J)
    assert np.array_equal(seld_augment.cell_source(0, I, J), cells) and np.array_equal(seld_augment.cell_dest(0, I, J), cells)
    assert len({seld_augment.cell_dest(p, I, J).tobytes() for p in range(16)}) == 16           # 16 distinct transforms
    tables = [seld_augment.cell_dest(p, I, J) for p in range(16)]
    signed = [_signed_matrix(seld_augment.channel_table("logmel_iv", 7, "WYZX")[p]) for p in range(16)]
    for p in range(16):
        dest, src = tables[p], seld_augment.cell_source(p, I, J)
        assert np.array_equal(np.sort(dest), cells) and np.array_equal(np.sort(src), cells)
        assert np.array_equal(dest[src], cells)
        # an inverse among the 16, the same one on the cells and on the channels
        inverses = [q for q in range(16) if np.array_equal(tables[q][dest], cells)]
        assert len(inverses) == 1
        assert np.array_equal(signed[inverses[0]] @ signed[p], np.eye(3, dtype=int))
        # closed under composition, again the same product on both sides
        for r in (3, 6, 9):
            product = [q for q in range(16) if np.array_equal(tables[q], tables[r][dest])]
            assert len(product) == 1
            assert np.array_equal(signed[product[0]], signed[r] @ signed[p])
    assert seld_augment.decode(11) == (1, 1, 1)
    with pytest.raises(ValueError):
        seld_augment.cell_dest(1, 18, 34)                                                       # J % 4 != 0


@pytest.mark.parametrize("order", ["WYZX", "WXYZ"])
@pytest.mark.parametrize("feature_set,channels", [("logmel", 4), ("logmel_iv", 7)])
def test_channel_tables_are_signed_permutations_that_fix_w(order, feature_set, channels):
    import seld_augment
    table = seld_augment.channel_table(feature_set, channels, order)
    assert table.shape == (16, channels) and table.dtype == np.uint8
    assert np.array_equal(table[0], np.arange(channels))                                        # p = 0: identity, no sign
    for p in range(16):
        src, neg = table[p] & 0x7f, table[p] & 0x80
        assert src[0] == 0 and not neg[0]                                                       # W never changes
        assert sorted(src[:4]) == [0, 1, 2, 3] and not neg[:4].any()                            # log-mel: the sign drops out
        if channels == 7:
            assert sorted(src[4:]) == [4, 5, 6] and np.array_equal(src[4:] - 3, src[1:4])       # IV follows its axis
        # against the independent restatement: transform a field of distinct "signals" and read off who went where
        ch = {letter: n for n, letter in enumerate(order)}
        x, y, z = augment_ref.field_transformed(ch["X"] * 1.0, ch["Y"] * 1.0, ch["Z"] * 1.0, p)
        for letter, value in (("X", x), ("Y", y), ("Z", z)):
            c = ch[letter]
            assert src[c] == abs(value), (p, letter)
            if channels == 7:
                assert bool(neg[3 + c]) == (np.copysign(1.0, value) < 0), (p, letter)
    assert len({table[p].tobytes() for p in range(16)}) == (16 if channels == 7 else 2)         # log-mel alone sees only the X-Y swap


def test_channel_tables_of_other_feature_sets_are_identity_and_refused():
    import seld_augment
    assert np.array_equal(seld_augment.channel_table("logmel_gcc", 36, "WYZX"), np.tile(np.arange(36, dtype=np.uint8), (16, 1)))
    assert seld_augment.freq_mask_channels("logmel_gcc", 36) == 8 and seld_augment.freq_mask_channels("logmel_gcc", 10) == 4
    assert seld_augment.freq_mask_channels("logmel", 4) == 4 and seld_augment.freq_mask_channels("logmel_iv", 7) == 7
    with pytest.raises(ValueError, match="AUGMENT_SPATIAL"):
        seld_augment.check_settings(_cfg(AUGMENT_SPATIAL=True), "logmel_gcc", 36)
    with pytest.raises(ValueError, match="AUGMENT_SPATIAL"):
        seld_augment.check_settings(_cfg(AUGMENT_SPATIAL=True), "logmel", 8)
    seld_augment.check_settings(_cfg(AUGMENT_TIME_MASKS=2, AUGMENT_TIME_MASK_MAX=20), "logmel_gcc", 36)   # masks: every set
    with pytest.raises(ValueError):
        seld_augment.check_settings(_cfg(AUGMENT_FREQ_MASKS=3))
    with pytest.raises(ValueError, match="FOA_CHANNEL_ORDER"):
        seld_augment.check_settings(_cfg(FOA_CHANNEL_ORDER="XYZW"))


# ---------------------------------------------------------------------------------------------- 3. draw

def test_draw_depends_on_seed_epoch_and_window_only():
    import seld_augment
    cfg = _cfg(AUGMENT_SPATIAL=True, AUGMENT_TIME_MASKS=2, AUGMENT_TIME_MASK_MAX=40, AUGMENT_FREQ_MASKS=2, AUGMENT_FREQ_MASK_MAX=12)
    every = seld_augment.draw(5, 1, np.arange(3000), cfg)
    assert every.shape == (3000, 12) and every.dtype == np.int32
    # whatever batch or rank asks for a window gets the same row: other batch sizes, a shuffled order, a rank's shard,
    # a window repeated by the wrap padding
    order = np.random.default_rng(0).permutation(3000)
    assert np.array_equal(seld_augment.draw(5, 1, order[:32], cfg), every[order[:32]])
    assert np.array_equal(seld_augment.draw(5, 1, order[1::4][:7], cfg), every[order[1::4][:7]])
    assert np.array_equal(seld_augment.draw(5, 1, [17, 2999, 17], cfg), every[[17, 2999, 17]])
    # another epoch or seed: other transforms
    assert not np.array_equal(seld_augment.draw(5, 2, np.arange(3000), cfg), every)
    assert not np.array_equal(seld_augment.draw(6, 1, np.arange(3000), cfg), every)
    # bounds
    assert every[:, 0].min() == 0 and every[:, 0].max() == 15 and len(np.unique(every[:, 0])) == 16
    counts = np.bincount(every[:, 0], minlength=16)
    assert counts.min() > 120 and counts.max() < 260                                 # uniform: 187.5 expected, sigma 13
    for first, axis, longest in ((1, 250, 40), (3, 250, 40), (5, 64, 12), (7, 64, 12)):
        start, length = every[:, first], every[:, first + 1]
        assert start.min() >= 0 and length.min() == 0 and length.max() == longest and (start + length).max() <= axis
        assert (start + length).max() == axis                                        # masks that touch the end occur
    assert not every[:, 9:].any()
    # a longest mask beyond the axis is clipped to it
    wide = seld_augment.draw(1, 1, np.arange(200), _cfg(AUGMENT_FREQ_MASKS=1, AUGMENT_FREQ_MASK_MAX=500))
    assert wide[:, 6].max() <= 64 and (wide[:, 5] + wide[:, 6]).max() <= 64 and not wide[:, 0].any()
    # one switch at a time touches its own fields only
    only_spatial = seld_augment.draw(5, 1, np.arange(50), _cfg(AUGMENT_SPATIAL=True))
    assert only_spatial[:, 0].any() and not only_spatial[:, 1:].any()
    only_time = seld_augment.draw(5, 1, np.arange(50), _cfg(AUGMENT_TIME_MASKS=1, AUGMENT_TIME_MASK_MAX=30))
    assert only_time[:, 2].any() and not only_time[:, 0].any() and not only_time[:, 3:].any()
    # everything off: identity rows
    off = seld_augment.draw(5, 1, np.arange(50), _cfg())
    assert off.shape == (50, 12) and not off.any() and not seld_augment.enabled(_cfg())
    assert np.array_equal(off, seld_augment.identity_rows(50))


def test_config_defaults_are_off():
    import seld_augment
    from config import Config
    cfg = Config
    assert cfg.AUGMENT_SPATIAL is False and cfg.AUGMENT_TIME_MASKS == 0 and cfg.AUGMENT_FREQ_MASKS == 0
    assert cfg.AUGMENT_TIME_MASK_MAX == 0 and cfg.AUGMENT_FREQ_MASK_MAX == 0 and cfg.AUGMENT_MASK_VALUE == 0.0
    assert cfg.FOA_CHANNEL_ORDER == "WYZX" and not seld_augment.enabled(cfg)


def test_host_parameter_table_is_validated():
    import seld_native
    ok = np.zeros((3, 12), dtype=np.int32)
    ok[1] = (15, 0, 250, 249, 1, 0, 64, 63, 1, 0, 0, 0)
    for column, value in ((0, 16), (0, -1), (1, -1), (2, 251), (3, 250), (6, 65), (7, 64)):
        bad = ok.copy()
        bad[1, column] = value
        if column in (3, 7):
            bad[1, column + 1] = 1
        with pytest.raises(ValueError):
            seld_native.augment_params(bad, 3, 250, "cpu")
    with pytest.raises(ValueError):
        seld_native.augment_params(ok[:2], 3, 250, "cpu")
    assert seld_native.augment_params(ok, 3, 250, "cpu").dtype == torch.int32


# ---------------------------------------------------------------------------------------------- 4. compiler resource check

def test_augment_kernels_use_no_scratch():
    """Same method as test_hot_kernels_do_not_spill: the compiler's own report for gfx950 must show 0 bytes of scratch per
    lane for the feature kernel and both instantiations of the label kernel (the by-value channel table is indexed from
    kernel-argument memory, not copied to a stack)."""
    import hip_resources
    found = {k: v["scratch"] for k, v in hip_resources.report(CSRC / "augment.hip").items()}
    for kernel in ("gather_augment_kernel", "permute_mask_kernel"):
        hits = {k: v for k, v in found.items() if kernel in k}
        assert hits, (kernel, sorted(found))
        assert all(v == 0 for v in hits.values()), hits


# ---------------------------------------------------------------------------------------------- 5. host-path error

class _Windows(torch.utils.data.Dataset):
    def __len__(self):
        return 8

    def __getitem__(self, i):
        return torch.zeros(2, 4, 64), torch.zeros(2, 648, 14)


@pytest.mark.parametrize("switch,value", [("AUGMENT_SPATIAL", True), ("AUGMENT_TIME_MASKS", 1), ("AUGMENT_FREQ_MASKS", 2)])
def test_host_loader_path_refuses_augmentation(switch, value):
    """The augmentation is done by the device gather; the stock DataLoader path has no CPU version of it and says so."""
    import trainer
    from config import Config
    loader = torch.utils.data.DataLoader(_Windows(), batch_size=4)
    trainer.LoaderFeed(loader, torch.device("cpu"))                         # switches off: fine
    saved = getattr(Config, switch)
    try:
        setattr(Config, switch, value)
        with pytest.raises(RuntimeError, match=switch):
            trainer.LoaderFeed(loader, torch.device("cpu"))
        with pytest.raises(RuntimeError, match="no CPU implementation"):
            trainer.make_feed(loader, torch.device("cpu"), 0, 1)
    finally:
        setattr(Config, switch, saved)
    trainer.make_feed(loader, torch.device("cpu"), 0, 1)
