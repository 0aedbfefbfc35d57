"""GPU tests of class-balanced window sampling: both kernels of csrc/balance.hip through the C ABI,
bit-exact against tests/balance_ref.py; what the two entry points refuse; SELDDataset.window_class_counts; and the training
feed's order, batches and augmentation keys with the switch on -- and its unchanged order with the switch off."""
import ctypes

import numpy as np
import pytest
import torch
from torch.utils.data import DataLoader

import balance_ref as ref
from oracle import features as ofeat
from oracle import labels as olab

pytestmark = pytest.mark.gpu

CELLS = 648
INVALID, UNSUPPORTED = -1, -4
ROW_SENTINEL, COUNT_SENTINEL = 0xABCD, -7777
PAD = 40                                                   # sentinel elements / rows behind every output
ROWS = (1, 63, 64, 65, 250, 251, 613)
WINDOWS = ((250, 50), (7, 3), (64, 64), (65, 1), (1000, 100))       # the last: a window longer than every timeline here
FOURTEEN_CELLS = (0, 7, 8, 63, 64, 300, 511, 512, 519, 520, 600, 640, 646, 647)


def _masks(total):
    """name -> uint16 [total, 648]"""
    rng = np.random.default_rng(total)
    out = {"zero": np.zeros((total, CELLS), np.uint16)}
    first = out["zero"].copy()
    first[::2, 0] = 1 << 3
    out["cell 0 only"] = first
    last = out["zero"].copy()
    last[:, CELLS - 1] = 1 << 9
    last[total // 2, CELLS - 1] = 1 << 2
    out["cell 647 only"] = last
    ragged = out["zero"].copy()                            # cells 512..647: the 17 chunks of the ragged second load
    for t in range(total):
        ragged[t, 512 + (t * 37) % 136] = 1 << (t % 13)
        ragged[t, 512 + 8 * (t % 17)] |= 1 << ((t // 3) % 13)
    out["cells 512..647"] = ragged
    fourteen = out["zero"].copy()
    for bit, cell in enumerate(FOURTEEN_CELLS):
        fourteen[total // 2, cell] = 1 << bit
    out["14 bits in 14 cells of one row"] = fourteen
    thirteen = out["zero"].copy()
    thirteen[total // 3:, 100] = 1 << 13
    thirteen[::5, 640] = 1 << 0
    out["bit 13"] = thirteen
    ignored = out["zero"].copy()
    ignored[:, 5] = 1 << 14
    ignored[::3, 530] = 1 << 15
    ignored[::4, 200] = (1 << 15) | (1 << 6)
    out["bits 14 and 15"] = ignored
    sparse = np.where(rng.random((total, CELLS)) < 0.003, 1 << rng.integers(0, 14, (total, CELLS)), 0).astype(np.uint16)
    sparse[rng.random(total) < 0.4] = 0                    # silent frames
    out["random sparse"] = sparse
    return out


@pytest.fixture(scope="module")
def library(gpu_device):
    import seld_native
    seld_native.ensure_init(gpu_device)
    return seld_native.load_library(), seld_native._stream_ptr(gpu_device)


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


@pytest.mark.parametrize("total", ROWS)
def test_kernels_are_bit_equal_to_the_restatement(gpu_device, library, total):
    lib, stream = library
    for name, mask in _masks(total).items():
        want_rows = ref.frame_class_mask(mask)
        mask_d = torch.from_numpy(mask).to(gpu_device)
        assert mask_d.data_ptr() % 16 == 0
        rows_d = torch.full((total + PAD,), ROW_SENTINEL, dtype=torch.uint16, device=gpu_device)
        assert lib.seld_frame_class_mask(_ptr(mask_d), total, CELLS, _ptr(rows_d), stream) == 0, lib.seld_last_error()
        got = rows_d.cpu().numpy()
        assert np.array_equal(got[:total], want_rows), name
        assert (got[total:] == ROW_SENTINEL).all(), name                 # every row written, nothing behind them
        classes = (14, 13, 1) if name in ("bit 13", "bits 14 and 15", "14 bits in 14 cells of one row") else (14,)
        for window, hop in WINDOWS:
            n = (total + hop - 1) // hop
            for num_classes, n_windows in [(c, n) for c in classes] + [(14, 1)]:
                want = ref.window_class_frames(want_rows, window, hop, n_windows, num_classes)
                counts_d = torch.full((n_windows + PAD, 16), COUNT_SENTINEL, dtype=torch.int32, device=gpu_device)
                rc = lib.seld_window_class_frames(_ptr(rows_d), total, window, hop, n_windows, num_classes, _ptr(counts_d),
                                                  stream)
                assert rc == 0, lib.seld_last_error()
                got_counts = counts_d.cpu().numpy()
                assert np.array_equal(got_counts[:n_windows], want), (name, window, hop, num_classes)
                assert (got_counts[n_windows:] == COUNT_SENTINEL).all(), (name, window, hop)
        if name == "bits 14 and 15":                                     # the OR keeps them, the counts ignore them
            assert (want_rows & 0xC000).any()
            assert ref.window_class_frames(want_rows, 250, 50, 1, 14)[0, 14] == len(want_rows[:250][::4])
        if name == "14 bits in 14 cells of one row":
            assert want_rows[total // 2] == (1 << 14) - 1


@pytest.mark.parametrize("cells", [8, 512, 520, 1024, 1032, 1544, 2048])
def test_frame_words_at_other_row_lengths(gpu_device, library, cells):
    """The other instantiations of the frame kernel (1 to 4 loads per row; 648 cells take two): a full last load, a last
    load of one lane, and a single chunk per row."""
    lib, stream = library
    rng = np.random.default_rng(cells)
    total = 67
    mask = np.where(rng.random((total, cells)) < 0.01, 1 << rng.integers(0, 16, (total, cells)), 0).astype(np.uint16)
    mask[:, cells - 1] |= (np.arange(total) % 3 == 0).astype(np.uint16) << 11       # the row's last cell decides some rows
    mask[5] = 0
    mask_d = torch.from_numpy(mask).to(gpu_device)
    rows_d = torch.full((total + PAD,), ROW_SENTINEL, dtype=torch.uint16, device=gpu_device)
    assert lib.seld_frame_class_mask(_ptr(mask_d), total, cells, _ptr(rows_d), stream) == 0, lib.seld_last_error()
    got = rows_d.cpu().numpy()
    assert np.array_equal(got[:total], ref.frame_class_mask(mask)) and (got[total:] == ROW_SENTINEL).all()


def test_the_cases_reach_the_ragged_load_and_several_waves():
    """What the shapes above are for: 648 cells = 81 chunks = one full 64-lane load and 17 lanes of a second; 613 rows are
    154 groups of four rows (the last one ragged), more than one block of four wavefronts."""
    assert CELLS // 8 == 64 + 17 and 512 // 8 == 64
    assert sorted(FOURTEEN_CELLS) == list(FOURTEEN_CELLS) and len(set(FOURTEEN_CELLS)) == 14
    assert sum(c >= 512 for c in FOURTEEN_CELLS) >= 5 and 613 % 4 == 1 and 613 // 4 > 4 * 4


# ------------------------------------------------------------------------------------------------ refusals

FRAME_CASES = [("null mask", {"mask": None}, INVALID), ("null frame_mask", {"out": None}, INVALID),
               ("total_rows = 0", {"total_rows": 0}, INVALID), ("total_rows = -3", {"total_rows": -3}, INVALID),
               ("cells = 0", {"cells": 0}, INVALID), ("cells = -8", {"cells": -8}, INVALID),
               ("cells = 644", {"cells": 644}, UNSUPPORTED), ("cells = 4", {"cells": 4}, UNSUPPORTED),
               ("cells = 2056", {"cells": 2056}, UNSUPPORTED), ("mask 2 bytes off", {"mask": "offset"}, UNSUPPORTED),
               ("total_rows = 2^31", {"total_rows": 1 << 31}, UNSUPPORTED)]
WINDOW_CASES = [("null frame_mask", {"rows": None}, INVALID), ("null counts", {"out": None}, INVALID),
                ("total_rows = 0", {"total_rows": 0}, INVALID), ("window = 0", {"window": 0}, INVALID),
                ("hop = 0", {"hop": 0}, INVALID), ("hop = -1", {"hop": -1}, INVALID),
                ("n_windows = 0", {"n_windows": 0}, INVALID), ("n_windows = -2", {"n_windows": -2}, INVALID),
                ("last window starts at the end", {"n_windows": 3}, INVALID),          # (3 - 1) * 50 >= 100
                ("last window starts behind the end", {"n_windows": 2, "hop": 101}, INVALID),
                ("num_classes = 0", {"num_classes": 0}, INVALID), ("num_classes = 15", {"num_classes": 15}, INVALID),
                ("window = 2^31", {"window": 1 << 31}, UNSUPPORTED),
                ("window = 2^31 - 64", {"window": (1 << 31) - 64}, UNSUPPORTED),
                ("n_windows = 2^31 + 1", {"n_windows": (1 << 31) + 1, "hop": 1, "total_rows": (1 << 31) + 5}, UNSUPPORTED)]


@pytest.fixture(scope="module")
def refusal_buffers(gpu_device, library):
    mask = torch.full((100, CELLS), 1, dtype=torch.uint16, device=gpu_device)
    rows = torch.full((100,), 1, dtype=torch.uint16, device=gpu_device)
    out_rows = torch.full((128,), ROW_SENTINEL, dtype=torch.uint16, device=gpu_device)
    out_counts = torch.full((8, 16), COUNT_SENTINEL, dtype=torch.int32, device=gpu_device)
    yield mask, rows, out_rows, out_counts
    torch.cuda.synchronize(gpu_device)
    assert bool((out_rows == ROW_SENTINEL).all()) and bool((out_counts == COUNT_SENTINEL).all())


@pytest.mark.parametrize("case,overrides,expected", FRAME_CASES, ids=[c[0] for c in FRAME_CASES])
def test_frame_entry_point_refuses(library, refusal_buffers, case, overrides, expected):
    lib, stream = library
    mask, _, out_rows, _ = refusal_buffers
    a = {"mask": _ptr(mask), "total_rows": 100, "cells": CELLS, "out": _ptr(out_rows)}
    a.update(overrides)
    if a["mask"] == "offset":
        a["mask"] = ctypes.c_void_p(mask.data_ptr() + 2)
    rc = lib.seld_frame_class_mask(a["mask"], a["total_rows"], a["cells"], a["out"], stream)
    print(case, rc, lib.seld_last_error())
    assert rc == expected and lib.seld_last_error().startswith(b"seld_frame_class_mask:")
    torch.cuda.synchronize()
    assert bool((out_rows == ROW_SENTINEL).all())                         # refused before anything was launched


@pytest.mark.parametrize("case,overrides,expected", WINDOW_CASES, ids=[c[0] for c in WINDOW_CASES])
def test_window_entry_point_refuses(library, refusal_buffers, case, overrides, expected):
    lib, stream = library
    _, rows, _, out_counts = refusal_buffers
    a = {"rows": _ptr(rows), "total_rows": 100, "window": 250, "hop": 50, "n_windows": 2, "num_classes": 14,
         "out": _ptr(out_counts)}
    a.update(overrides)
    rc = lib.seld_window_class_frames(a["rows"], a["total_rows"], a["window"], a["hop"], a["n_windows"], a["num_classes"],
                                      a["out"], stream)
    print(case, rc, lib.seld_last_error())
    assert rc == expected and lib.seld_last_error().startswith(b"seld_window_class_frames:")
    torch.cuda.synchronize()
    assert bool((out_counts == COUNT_SENTINEL).all())


def test_the_good_calls_of_the_refusal_tables_run(library, gpu_device):
    """The calls the tables override are accepted as they stand (on buffers of their own)."""
    lib, stream = library
    mask = torch.full((100, CELLS), 1 << 4, dtype=torch.uint16, device=gpu_device)
    rows = torch.zeros(100, dtype=torch.uint16, device=gpu_device)
    counts = torch.zeros((2, 16), dtype=torch.int32, device=gpu_device)
    assert lib.seld_frame_class_mask(_ptr(mask), 100, CELLS, _ptr(rows), stream) == 0
    assert lib.seld_window_class_frames(_ptr(rows), 100, 250, 50, 2, 14, _ptr(counts), stream) == 0
    want = np.zeros((2, 16), np.int32)
    want[:, 4], want[:, 14], want[:, 15] = (100, 50), (100, 50), (100, 50)
    assert np.array_equal(counts.cpu().numpy(), want)


# ------------------------------------------------------------------------------------------------ dataset

def test_dataset_counts_equal_the_restatement_on_its_own_mask(gpu_device):
    import dataset
    clips = [ofeat.synth_pcm(i, 4, 24000 * 6 + 37 * i, "noise") for i in range(2)]
    rows = [olab.synth_metadata(i, meta_frames=60) for i in range(2)]
    ds = dataset.SELDDataset.from_pcm(clips, rows, device=gpu_device)
    counts = ds.window_class_counts()
    want = ref.window_class_frames(ref.frame_class_mask(ds._mask_host), ds.window_length_frames, ds.hop_length_frames,
                                   len(ds), ds.num_classes)
    assert isinstance(counts, np.ndarray) and counts.dtype == np.int32 and counts.shape == (len(ds), 16)
    assert np.array_equal(counts, want)
    assert counts[-1, 15] < ds.window_length_frames and counts[0, 15] == ds.window_length_frames     # short tail windows
    assert counts[:, :13].any() and not counts[:, 13].any()
    assert ds.window_class_counts() is counts                              # cached
    host_only = dataset.SELDDataset.__new__(dataset.SELDDataset)
    host_only.mask_tm = None
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        host_only.window_class_counts()


# ------------------------------------------------------------------------------------------------ feed

class _Switches:
    """Sets switches on trainer's own Config INSTANCE (what the feed reads; an attribute another test left on the instance
    would shadow a class attribute) and puts them back afterwards."""

    def __init__(self):
        import trainer
        object.__setattr__(self, "config", trainer.config)
        object.__setattr__(self, "_saved", {})

    def __setattr__(self, name, value):
        own = vars(self.config)
        self._saved.setdefault(name, (name in own, own.get(name)))
        setattr(self.config, name, value)

    def __getattr__(self, name):
        return getattr(self.config, name)

    def restore(self):
        for name, (was_own, value) in self._saved.items():
            if was_own:
                setattr(self.config, name, value)
            else:                                          # leave no instance attribute behind: it would shadow the class's
                vars(self.config).pop(name, None)


@pytest.fixture
def class_config():
    switches = _Switches()
    yield switches
    switches.restore()


def _skewed_dataset(device):
    """Two 12 s clips = 1200 frames = 24 windows: class 0 through most of the first clip, class 4 for 0.6 s, class 9 for
    0.2 s beside class 0, the second half of the second clip silent."""
    import dataset
    clips = [ofeat.synth_pcm(20 + i, 4, 24000 * 12, "noise") for i in range(2)]
    first = [(t, 0, 0, 30, 10) for t in range(5, 100)] + [(t, 9, 1, -60, 0) for t in range(40, 42)]
    second = [(t, 4, 0, 120, -20) for t in range(10, 16)] + [(t, 0, 0, 0, 0) for t in range(30, 45)]
    rows = [np.asarray(first, dtype=np.int64), np.asarray(second, dtype=np.int64)]
    return dataset.SELDDataset.from_pcm(clips, rows, device=device)


def _equal(got, want):
    return all(torch.equal(g.view(torch.int32) if g.dtype == torch.float32 else g.view(torch.int16),
                           w.view(torch.int32) if w.dtype == torch.float32 else w.view(torch.int16))
               for g, w in zip(got, want))


def test_feed_order_batches_and_augmentation_keys(gpu_device, class_config):
    import seld_augment
    import seld_balance
    import trainer
    ds = _skewed_dataset(gpu_device)
    loader = DataLoader(ds, batch_size=6, shuffle=True)
    seed = 4242

    # switch off: the permutation, unchanged, whoever asks
    off = trainer.DeviceFeed(loader, gpu_device, 0, 1, seed=seed)
    assert not off.balanced
    for epoch in (1, 2):
        assert off._order(epoch) == trainer.epoch_order(len(ds), True, seed, epoch)
        assert sorted(off._order(epoch)) == list(range(len(ds)))
    plain = [ds.device_batch(idx) for idx in trainer.batched(off._order(1), 6, False)]
    assert all(_equal(g, w) for g, w in zip(off.batches(1, balanced=True), plain))

    class_config.BALANCED_SAMPLING, class_config.SEED = True, seed
    class_config.BALANCE_SILENT_SHARE = 0.1
    s = seld_balance.settings(trainer.config)
    counts = ds.window_class_counts()
    k = seld_balance.window_weights(counts, s)
    assert len(set(k.tolist())) >= 3 and len(k) == len(ds) == 24
    feed = trainer.make_feed(loader, gpu_device, 0, 1)
    assert isinstance(feed, trainer.DeviceFeed) and feed.balanced and feed.seed == seed and len(feed) == len(off) == 4
    assert not trainer.make_feed(DataLoader(ds, batch_size=6, shuffle=False), gpu_device, 0, 1).balanced
    report = trainer.log_balanced_sampling(feed)
    assert abs(report["silent_expected"] - 0.1) < 1e-6 and np.array_equal(feed.balance_table(), k)
    repeated = 0
    for epoch in (1, 2, 3):
        want = seld_balance.order(k, seed, epoch).tolist()
        assert feed._order(epoch) == want
        assert feed._order(epoch, balanced=False) == trainer.epoch_order(len(ds), True, seed, epoch)
        lists = trainer.batched(want, 6, False)
        repeated += sum(len(set(idx)) < len(idx) for idx in lists)
        got = list(feed.batches(epoch, balanced=True))
        assert len(got) == len(lists) == len(feed)
        for g, idx in zip(got, lists):
            assert _equal(g, ds.device_batch(idx))
        # only the caller that asks gets the balanced order (evaluation loops never do)
        assert _equal(next(iter(feed.batches(epoch))), ds.device_batch(trainer.epoch_order(len(ds), True, seed, epoch)[:6]))
    assert repeated >= 1                                                   # a batch that holds the same window twice

    # augmentation: every draw is keyed on its position in the epoch's global order, not on the window index
    class_config.AUGMENT_SPATIAL = True
    class_config.AUGMENT_TIME_MASKS, class_config.AUGMENT_TIME_MASK_MAX = 2, 40
    window = ds.window_length_frames
    for rank, world in ((0, 1), (1, 2)):
        fed = trainer.DeviceFeed(loader, gpu_device, rank, world, seed=seed)
        fed._balance_k = k                                                 # (no process group here: the table as agreed)
        order = seld_balance.order(k, seed, 1).tolist()[rank::world]
        assert fed._order(1) == order
        got = list(fed.batches(1, augment=True, balanced=True))
        position = 0
        for g, idx in zip(got, trainer.batched(order, 6, False)):
            keys = [rank + world * (position + j) for j in range(len(idx))]
            position += len(idx)
            rows = seld_augment.draw(seed, 1, idx, trainer.config, window=window, keys=keys)
            assert _equal(g, ds.device_batch(idx, augment=rows))
        assert position == len(order)
    order = seld_balance.order(k, seed, 1).tolist()
    twice = next(w for w in order if order.count(w) > 1)
    a, b = [p for p, w in enumerate(order) if w == twice][:2]
    by_position = seld_augment.draw(seed, 1, [twice, twice], trainer.config, window=window, keys=[a, b])
    by_index = seld_augment.draw(seed, 1, [twice, twice], trainer.config, window=window)
    assert not np.array_equal(by_position[0], by_position[1]) and np.array_equal(by_index[0], by_index[1])


def test_out_of_range_settings_are_refused_when_the_feed_is_built(gpu_device, class_config):
    import trainer
    ds = _skewed_dataset(gpu_device)
    loader = DataLoader(ds, batch_size=6, shuffle=True)
    class_config.BALANCED_SAMPLING = True
    for name, bad in (("BALANCE_POWER", 1.5), ("BALANCE_SILENT_SHARE", 1.0), ("BALANCE_MIN_FRAMES", 0)):
        saved = getattr(class_config, name)
        setattr(class_config, name, bad)
        with pytest.raises(ValueError, match=name):
            trainer.make_feed(loader, gpu_device, 0, 1)
        setattr(class_config, name, saved)
    trainer.make_feed(loader, gpu_device, 0, 1)
    class_config.BALANCE_MIN_FRAMES = 250 * 2                              # no class lasts that long: nothing to balance
    with pytest.raises(ValueError, match="no window holds a class"):
        trainer.make_feed(loader, gpu_device, 0, 1)._order(1)
