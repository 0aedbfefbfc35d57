"""GPU tests of the training augmentation in the device window gather (csrc/augment.hip, seld_augment.py; DESIGN.md section
11): the kernels bit-exact against tests/augment_ref.py, identity rows against the plain gather, the tables against the
physics (a channel-transformed clip with transformed metadata), and the training path."""
import numpy as np
import pytest
import torch
from torch.utils.data import DataLoader

import augment_ref
from oracle import features as ofeat
from oracle import labels as olab

pytestmark = pytest.mark.gpu

WINDOW = 250
I, J = 18, 36


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else a.dtype)


def _timeline(seed, total, channels):
    """A synthetic device timeline: signed floats with zeros and negative zeros mixed in, sparse uint16 class masks."""
    rng = np.random.default_rng(seed)
    spec = (rng.standard_normal((total, channels, 64)) * 30).astype(np.float32)
    spec[rng.random(spec.shape) < 0.01] = 0.0
    spec[rng.random(spec.shape) < 0.01] = -0.0
    mask = np.where(rng.random((total, I * J)) < 0.03, rng.integers(1, 1 << 13, (total, I * J)), 0).astype(np.uint16)
    return spec, mask


def _params(rng, patterns, window=WINDOW):
    """One row per pattern given, cycling through the mask shapes the issue lists: random, empty, full-width, end-touching.
    Slot [9], the azimuth step of the rotating entry points, holds a seeded value in 0..35: the restatement and the two
    entry points under test here ignore it (a generator of its own, so the masks drawn from ``rng`` are what they were)."""
    rows = np.zeros((len(patterns), 12), dtype=np.int32)
    steps = np.random.default_rng(len(patterns)).integers(0, 36, len(patterns))
    for r, p in enumerate(patterns):
        kind = r % 5
        if kind == 0:                                    # random
            tl, fl = rng.integers(0, 60, 2), rng.integers(0, 20, 2)
            t = [rng.integers(0, window - n + 1) for n in tl]
            f = [rng.integers(0, 64 - n + 1) for n in fl]
        elif kind == 1:                                  # empty (zero length, any start)
            t, tl, f, fl = [10, 249], [0, 0], [0, 63], [0, 0]
        elif kind == 2:                                  # full width in frequency, one long and one one-frame time mask
            t, tl, f, fl = [0, 249], [100, 1], [0, 5], [64, 3]
        elif kind == 3:                                  # touching the ends of both axes, overlapping pairs
            t, tl, f, fl = [window - 30, window - 10], [30, 10], [64 - 7, 0], [7, 1]
        else:                                            # the whole window in time
            t, tl, f, fl = [0, 0], [window, 0], [3, 60], [2, 4]
        rows[r] = (p, t[0], tl[0], t[1], tl[1], f[0], fl[0], f[1], fl[1], steps[r], 0, 0)
    return rows


def _run(dev, spec, mask, starts, rows, table, freq_channels, mask_value, with_out):
    import seld_native
    spec_d, mask_d = torch.from_numpy(spec).to(dev), torch.from_numpy(mask).to(dev)
    starts_t = torch.as_tensor(np.asarray(starts, dtype=np.int64))
    params = seld_native.augment_params(rows, len(starts), WINDOW, dev)
    out_s = out_m = None
    if with_out:                                         # the static buffers of a captured step: pre-filled with garbage
        out_s = torch.full((len(starts), WINDOW) + spec.shape[1:], float("nan"), dtype=torch.float32, device=dev)
        out_m = torch.from_numpy(np.full((len(starts), WINDOW, I * J), 0xFFFF, dtype=np.uint16)).to(dev)
    got_s = seld_native.gather_windows_augment(spec_d, starts_t, WINDOW, params, table, freq_channels, mask_value, out=out_s)
    got_m = seld_native.gather_windows_permute(mask_d, starts_t, WINDOW, params, I, J, out=out_m)
    if with_out:
        assert got_s.data_ptr() == out_s.data_ptr() and got_m.data_ptr() == out_m.data_ptr()
    torch.cuda.synchronize()
    return got_s.cpu().numpy(), got_m.cpu().numpy()


# ------------------------------------------------------------------------------------------ 6. kernels vs augment_ref

@pytest.mark.parametrize("feature_set,channels,order", [("logmel", 4, "WYZX"), ("logmel", 4, "WXYZ"),
                                                        ("logmel_iv", 7, "WYZX"), ("logmel_iv", 7, "WXYZ")])
@pytest.mark.parametrize("mask_value,with_out", [(0.0, False), (-80.0, True)])
def test_kernels_match_the_restatement_all_patterns(gpu_device, feature_set, channels, order, mask_value, with_out):
    """All 16 patterns (twice, so every pattern meets several mask shapes), both channel orders, tail windows that run past
    the timeline, a window wholly past it, repeated and shuffled starts; fp32 features and uint16 labels, bit for bit."""
    import seld_augment
    total = 640
    spec, mask = _timeline(channels, total, channels)
    rng = np.random.default_rng(100 + channels)
    patterns = list(rng.permutation(16)) + list(rng.permutation(16)) + [5, 5]
    starts = list(rng.integers(0, total - WINDOW, len(patterns) - 8)) + [600, 450, 391, total - 1, total, total + 70, 0, 0]
    starts = [int(starts[i]) for i in rng.permutation(len(starts))]
    starts[-1] = starts[0]                                           # a repeated window with another transform
    rows = _params(rng, patterns)
    table = seld_augment.channel_table(feature_set, channels, order)
    got_s, got_m = _run(gpu_device, spec, mask, starts, rows, table, channels, mask_value, with_out)
    want_s, want_m = augment_ref.gather(spec, mask, starts, rows, WINDOW, table, channels, mask_value, I, J)
    assert np.array_equal(_bits(got_s), _bits(want_s))
    assert np.array_equal(got_m, want_m)
    assert (want_s == np.float32(mask_value)).any() and want_m.any()
    # a batch composed differently gives the same windows (output depends on (source, start, row) only)
    pick = [7, 3, 3, 20]
    sub_s, sub_m = _run(gpu_device, spec, mask, [starts[i] for i in pick], rows[pick], table, channels, mask_value, False)
    assert np.array_equal(_bits(sub_s), _bits(got_s[pick])) and np.array_equal(sub_m, got_m[pick])


@pytest.mark.parametrize("mask_value", [0.0, 1.5])
def test_kernels_match_the_restatement_masks_only_36_channels(gpu_device, mask_value):
    """8 log-mel + 28 GCC-PHAT channels: no channel swap is defined (pattern 0, identity table), time masks cover every
    channel, frequency masks only the 8 log-mel channels -- the 64-wide axis of a GCC-PHAT channel is lags."""
    import seld_augment
    total, channels = 420, 36
    spec, mask = _timeline(36, total, channels)
    rng = np.random.default_rng(36)
    starts = [0, 170, 171, 300, 419, 170, 50, 0, 399, 260]
    rows = _params(rng, [0] * len(starts))
    table = seld_augment.channel_table("logmel_gcc", channels)
    freq = seld_augment.freq_mask_channels("logmel_gcc", channels)
    assert freq == 8
    got_s, got_m = _run(gpu_device, spec, mask, starts, rows, table, freq, mask_value, True)
    want_s, want_m = augment_ref.gather(spec, mask, starts, rows, WINDOW, table, freq, mask_value, I, J)
    assert np.array_equal(_bits(got_s), _bits(want_s)) and np.array_equal(got_m, want_m)
    # the row with the full-width frequency mask: log-mel channels masked, GCC channels untouched outside the time masks
    full = got_s[2]
    assert (full[120:150, :8] == np.float32(mask_value)).all()
    assert np.array_equal(_bits(full[120:150, 8:]), _bits(spec[171 + 120:171 + 150, 8:]))


def test_c_abi_rejects_what_it_does_not_support(gpu_device):
    import seld_native
    dev = gpu_device
    params = seld_native.augment_params(np.zeros((1, 12), np.int32), 1, WINDOW, dev)
    starts = torch.zeros(1, dtype=torch.int64)
    with pytest.raises(seld_native.SeldNativeError, match="-4"):                    # J % 4 != 0: unsupported
        seld_native.gather_windows_permute(torch.from_numpy(np.zeros((300, 20 * 34), dtype=np.uint16)).to(dev),
                                           starts, WINDOW, params, 20, 34)
    bad = np.tile(np.arange(4, dtype=np.uint8), (16, 1))
    bad[3, 2] = 4                                                                    # names a channel that is not there
    with pytest.raises(seld_native.SeldNativeError, match="-1"):
        seld_native.gather_windows_augment(torch.zeros((300, 4, 64), device=dev), starts, WINDOW, params, bad)
    # a direct C caller's hostile row (the host check is bypassed by handing over a device tensor): the kernels reduce the
    # pattern modulo 16 and only compare the masks, so the result is the clamped transform and nothing outside is touched
    spec, mask = _timeline(1, 400, 4)
    hostile = torch.tensor([[16 + 3, -5, 2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1, -(2 ** 31), 2 ** 31 - 1, 70, 9, 1, 2, 3]],
                           dtype=torch.int64).to(torch.int32).to(dev)
    guard = torch.full((3, WINDOW, 4, 64), 7.0, device=dev)
    import seld_augment
    table = seld_augment.channel_table("logmel", 4)
    seld_native.gather_windows_augment(torch.from_numpy(spec).to(dev), torch.tensor([100]), WINDOW, hostile, table, 4, -1.0,
                                       out=guard[1:2])
    got_m = seld_native.gather_windows_permute(torch.from_numpy(mask).to(dev), torch.tensor([100]), WINDOW, hostile, I, J)
    torch.cuda.synchronize()
    assert (guard[0] == 7.0).all() and (guard[2] == 7.0).all()
    # pattern 19 & 15 = 3; time mask 0 = every frame from -5 on: the whole window is masked
    assert (guard[1] == -1.0).all()
    assert np.array_equal(got_m.cpu().numpy()[0], augment_ref.permute_cells(mask[100:350], 3))


# ------------------------------------------------------------------------------------------ 7. identity

def _clips(seed, count=2, dtype="float32"):
    clips, rows = [], []
    for n in range(count):
        pcm = ofeat.synth_pcm(seed + n, 4, 24000 * (7 + n) + 211 * n, "noise")
        pcm[1] = 0.6 * pcm[0] + 0.4 * pcm[1]                              # some coherence: intensity vectors are not ~0
        pcm[3] = -0.5 * pcm[0] + 0.5 * pcm[3]
        clips.append(ofeat.pcm_to_int16(pcm) if dtype == "int16" else pcm)
        rows.append(augment_ref.off_edge_rows(olab.synth_metadata(seed + n, meta_frames=75 + 10 * n)))
    return clips, rows


@pytest.fixture
def class_config():
    """Switches are class attributes (config.py is edited in place upstream; dataset.py and trainer.py each hold an instance)."""
    from config import Config
    names = ("FEATURE_SET", "FOA_CHANNEL_ORDER", "AUGMENT_SPATIAL", "AUGMENT_TIME_MASKS", "AUGMENT_TIME_MASK_MAX",
             "AUGMENT_FREQ_MASKS", "AUGMENT_FREQ_MASK_MAX", "AUGMENT_MASK_VALUE")
    saved = {k: getattr(Config, k) for k in names}
    yield Config
    for k, v in saved.items():
        setattr(Config, k, v)


@pytest.mark.parametrize("feature_set", ["logmel", "logmel_iv"])
def test_identity_rows_equal_the_plain_gather(gpu_device, class_config, feature_set):
    import dataset
    import seld_augment
    import seld_native
    class_config.FEATURE_SET = feature_set
    clips, rows = _clips(40, dtype="int16")
    ds = dataset.SELDDataset.from_pcm(clips, rows, device=gpu_device)
    idx = [len(ds) - 1, 0, 3, 3, len(ds) - 2, 1]
    plain_s, plain_m = ds.device_batch(idx)
    aug_s, aug_m = ds.device_batch(idx, augment=seld_augment.identity_rows(len(idx)))
    assert aug_s.dtype == plain_s.dtype and aug_s.shape == plain_s.shape and aug_m.dtype == torch.uint16
    assert np.array_equal(_bits(aug_s.cpu().numpy()), _bits(plain_s.cpu().numpy()))
    assert np.array_equal(aug_m.cpu().numpy(), plain_m.cpu().numpy())
    # and straight through the binding, out= buffers included
    starts = torch.as_tensor(ds.window_starts[idx])
    params = seld_native.augment_params(seld_augment.identity_rows(len(idx)), len(idx), WINDOW, gpu_device)
    buf = torch.empty_like(plain_s)
    seld_native.gather_windows_augment(ds.spec_tm, starts, WINDOW, params, None, out=buf)
    assert torch.equal(buf.view(torch.int32), plain_s.view(torch.int32))
    # augment=None is today's path; a table of the wrong shape is refused
    with pytest.raises(ValueError):
        ds.device_batch(idx, augment=seld_augment.identity_rows(len(idx) + 1))


# ------------------------------------------------------------------------------------------ 8. physical consistency

PHYSICAL_PATTERNS = [8, 2, 4, 6, 1, 15, 11]         # mirror; the three rotations; elevation flip; two combinations of all


@pytest.mark.parametrize("order", ["WYZX", "WXYZ"])
def test_augmented_windows_equal_the_windows_of_the_transformed_recording(gpu_device, class_config, order):
    """The test that shows the tables mean what they claim.  Dataset A: float32 4-channel clips and their metadata.  Dataset
    B(p): the channel-transformed clips (augment_ref.pcm_transformed) with (az', el') metadata, built from scratch through
    the feature and label kernels.  A's windows gathered with pattern p must equal B(p)'s plain windows:
      labels          bit-equal
      log-mel         bit-equal: the per-channel arithmetic is sign-symmetric (a negated channel has the same power bits)
      intensity       within the 1e-4 of tests/test_spatial_gpu.py of oracle foa_intensity_f64 run on the TRANSFORMED clip
                      (the energy sum |X|^2 + |Y|^2 + |Z|^2 may be taken in another order)."""
    import dataset
    class_config.FEATURE_SET = "logmel_iv"
    class_config.FOA_CHANNEL_ORDER = order
    clips, rows = _clips(60)
    ds_a = dataset.SELDDataset.from_pcm(clips, rows, device=gpu_device)
    idx = list(range(len(ds_a)))
    frames = [int(n) for n in ds_a.segments[:, 1]]
    assert ds_a.n_channels == 7 and sum(frames) == ds_a.total_frames
    for p in PHYSICAL_PATTERNS:
        t_clips = [torch.from_numpy(np.ascontiguousarray(augment_ref.pcm_transformed(c.numpy(), p, order))) for c in clips]
        t_rows = [augment_ref.rows_transformed(r, p) for r in rows]
        ds_b = dataset.SELDDataset.from_pcm(t_clips, t_rows, device=gpu_device)
        params = np.zeros((len(idx), 12), dtype=np.int32)
        params[:, 0] = p
        aug_s, aug_m = (t.cpu().numpy() for t in ds_a.device_batch(idx, augment=params))
        ref_s, ref_m = (t.cpu().numpy() for t in ds_b.device_batch(idx))
        plain_s, plain_m = (t.cpu().numpy() for t in ds_a.device_batch(idx))
        assert np.array_equal(aug_m, ref_m), p                                      # labels: bit-equal
        assert not np.array_equal(aug_m, plain_m) and ref_m.any()
        mel_same = np.array_equal(_bits(aug_s[:, :, :4]), _bits(ref_s[:, :, :4]))
        mel_diff = float(np.abs(aug_s[:, :, :4].astype(np.float64) - ref_s[:, :, :4]).max())
        # oracle intensity vectors of the transformed clips, cropped and concatenated like the timeline, then windowed
        iv_tm = np.concatenate([ofeat.foa_intensity_f64(c.numpy().astype(np.float64))[:, :, :n].transpose(2, 0, 1)
                                for c, n in zip(t_clips, frames)])                  # [total, 3, 64]
        iv_ref = np.zeros((len(idx), WINDOW, 3, 64))
        for b, i in enumerate(idx):
            s = int(ds_a.window_starts[i])
            n = min(WINDOW, ds_a.total_frames - s)
            iv_ref[b, :n] = iv_tm[s:s + n]
        iv_err = float(np.abs(aug_s[:, :, 4:] - iv_ref).max())
        iv_kernels = float(np.abs(aug_s[:, :, 4:].astype(np.float64) - ref_s[:, :, 4:]).max())
        print(f"order {order} pattern {p:2d}: log-mel bit-equal {mel_same} (max |diff| {mel_diff:.3e} dB); "
              f"IV vs float64 oracle of the transformed clip {iv_err:.3e}; IV augmented vs re-computed {iv_kernels:.3e}; "
              f"max |IV| {np.abs(iv_ref).max():.3f}")
        assert mel_same, (p, mel_diff)
        assert iv_err <= 1e-4, (p, iv_err)
        assert np.abs(iv_ref).max() > 0.1                                           # the vectors are not trivially ~0
        if p != 0:
            assert not np.array_equal(_bits(aug_s[:, :, 4:]), _bits(plain_s[:, :, 4:]))


def test_logmel_only_features_take_the_same_swap(gpu_device, class_config):
    """FEATURE_SET 'logmel' (the reference's features, 4 channels): int16 clips without -32768 (negating it would overflow),
    a quarter turn swaps the X and Y log-mel channels, labels move with it; bit-equal to the transformed recording."""
    import dataset
    class_config.FEATURE_SET = "logmel"
    clips, rows = _clips(80, dtype="int16")
    clips = [c.clamp(min=-32767) for c in clips]
    ds_a = dataset.SELDDataset.from_pcm(clips, rows, device=gpu_device)
    idx = list(range(len(ds_a)))
    for p in (2, 9, 14):
        t_clips = [torch.from_numpy(np.ascontiguousarray(augment_ref.pcm_transformed(c.numpy(), p, "WYZX"))) for c in clips]
        assert all(t.dtype == torch.int16 for t in t_clips)
        ds_b = dataset.SELDDataset.from_pcm(t_clips, [augment_ref.rows_transformed(r, p) for r in rows], device=gpu_device)
        params = np.zeros((len(idx), 12), dtype=np.int32)
        params[:, 0] = p
        aug_s, aug_m = ds_a.device_batch(idx, augment=params)
        ref_s, ref_m = ds_b.device_batch(idx)
        assert torch.equal(aug_m.view(torch.int16), ref_m.view(torch.int16)), p
        assert torch.equal(aug_s.view(torch.int32), ref_s.view(torch.int32)), p


# ------------------------------------------------------------------------------------------ 9. training path

def test_spatial_switch_is_refused_for_microphone_arrays_when_the_feed_is_built(gpu_device, class_config):
    import dataset
    import trainer
    class_config.FEATURE_SET = "logmel_gcc"
    clips = [ofeat.synth_pcm(3, 8, 24000 * 6, "noise")]
    ds = dataset.SELDDataset.from_pcm(clips, [olab.synth_metadata(3, meta_frames=60)], device=gpu_device)
    assert ds.n_channels == 36
    loader = DataLoader(ds, batch_size=2, shuffle=False)
    class_config.AUGMENT_TIME_MASKS, class_config.AUGMENT_TIME_MASK_MAX = 2, 25
    class_config.AUGMENT_FREQ_MASKS, class_config.AUGMENT_FREQ_MASK_MAX = 1, 10
    assert isinstance(trainer.make_feed(loader, gpu_device, 0, 1), trainer.DeviceFeed)  # masks work for every feature set
    feed = trainer.DeviceFeed(loader, gpu_device, 0, 1, seed=5)
    spec, mask = next(iter(feed.batches(1, augment=True)))
    plain_s, plain_m = ds.device_batch([0, 1])
    assert torch.equal(mask.view(torch.int16), plain_m.view(torch.int16)) and not torch.equal(spec, plain_s)
    changed = (spec != plain_s)
    assert changed[:, :, :8].any()
    for b in range(2):                                                    # GCC lags: time masks only (two of <= 25 frames)
        assert int(changed[b, :, 8:].any(dim=2).any(dim=1).sum()) <= 2 * 25
    class_config.AUGMENT_SPATIAL = True
    with pytest.raises(ValueError, match="AUGMENT_SPATIAL"):
        trainer.make_feed(loader, gpu_device, 0, 1)


def test_training_with_augmentation_is_reproducible_and_evaluation_is_untouched(gpu_device, class_config, tmp_path):
    """Two train_model runs (2 epochs, small CRNN, captured steps, SEED set) with the switches on give identical loss
    histories, which differ from the run with the switches off; a window's batch differs between epoch 1 and epoch 2; the
    evaluation feed of the same process returns un-augmented windows.  Dropout is off and the library convolutions run in
    their deterministic mode, so that the only thing that may differ between the runs is the augmentation."""
    import dataset
    import trainer
    cfg = trainer.config
    names = ("MODEL_TYPE", "CRNN_CNN_CHANNELS", "CRNN_RNN_HIDDEN", "CRNN_DROPOUT", "NUM_EPOCHS", "BATCH_SIZE", "SEED",
             "OUTPUT_PATH", "CHECKPOINT_PATH", "GRAPH_STEP", "DEVICE_FEED")
    saved = {k: getattr(cfg, k) for k in names}
    saved_det = torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark
    try:
        torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = True, False
        cfg.MODEL_TYPE, cfg.CRNN_CNN_CHANNELS, cfg.CRNN_RNN_HIDDEN, cfg.CRNN_DROPOUT = "crnn", [8, 8, 16, 16], 16, 0.0
        cfg.NUM_EPOCHS, cfg.BATCH_SIZE, cfg.SEED, cfg.GRAPH_STEP, cfg.DEVICE_FEED = 2, 4, 11, True, True
        cfg.OUTPUT_PATH, cfg.CHECKPOINT_PATH = tmp_path / "outputs", tmp_path / "checkpoints"
        cfg.OUTPUT_PATH.mkdir()
        cfg.CHECKPOINT_PATH.mkdir()
        class_config.FEATURE_SET = "logmel_iv"
        clips, rows = _clips(90, count=3)
        train_ds = dataset.SELDDataset.from_pcm(clips[:2], rows[:2], device=gpu_device)
        test_ds = dataset.SELDDataset.from_pcm(clips[2:], rows[2:], device=gpu_device)
        train_loader = DataLoader(train_ds, batch_size=cfg.BATCH_SIZE, shuffle=True)
        test_loader = DataLoader(test_ds, batch_size=cfg.BATCH_SIZE, shuffle=False)

        def run(on):
            class_config.AUGMENT_SPATIAL = on
            class_config.AUGMENT_TIME_MASKS, class_config.AUGMENT_TIME_MASK_MAX = (2, 40) if on else (0, 0)
            class_config.AUGMENT_FREQ_MASKS, class_config.AUGMENT_FREQ_MASK_MAX = (2, 12) if on else (0, 0)
            assert trainer.graph_step_enabled(gpu_device, 1)
            for old in cfg.CHECKPOINT_PATH.glob("*.pth"):
                old.unlink()
            _, history = trainer.train_model(train_loader=train_loader, test_loader=test_loader, device=gpu_device)
            assert history["total_epochs"] == 2 and history["config"]["batch_source"] == "DeviceFeed"
            return history["train_losses"], history["test_losses"]

        first, second, off = run(True), run(True), run(False)
        print("augmented:", first, "again:", second, "switches off:", off)
        assert np.isfinite(first[0]).all() and np.isfinite(first[1]).all()
        assert first == second                                            # identical loss histories
        assert first[0] != off[0]                                         # and the augmentation is really in the path

        # a window's batch differs between epoch 1 and epoch 2; the evaluation feed is un-augmented, in this same process
        run_on = (True, 2, 40, 2, 12)
        (class_config.AUGMENT_SPATIAL, class_config.AUGMENT_TIME_MASKS, class_config.AUGMENT_TIME_MASK_MAX,
         class_config.AUGMENT_FREQ_MASKS, class_config.AUGMENT_FREQ_MASK_MAX) = run_on
        ordered = DataLoader(train_ds, batch_size=len(train_ds), shuffle=False)
        feed = trainer.make_feed(ordered, gpu_device, 0, 1)
        e1 = [t.clone() for t in next(iter(feed.batches(1, augment=True)))]
        e1_again = [t.clone() for t in next(iter(feed.batches(1, augment=True)))]
        e2 = [t.clone() for t in next(iter(feed.batches(2, augment=True)))]
        assert torch.equal(e1[0].view(torch.int32), e1_again[0].view(torch.int32)) and torch.equal(e1[1].view(torch.int16), e1_again[1].view(torch.int16))
        for w in range(len(train_ds)):
            assert not torch.equal(e1[0][w], e2[0][w]), w
        plain = train_ds.device_batch(list(range(len(train_ds))))
        for got in (next(iter(feed.batches(1))), next(iter(feed.batches(0, augment=False)))):
            assert torch.equal(got[0].view(torch.int32), plain[0].view(torch.int32))
            assert torch.equal(got[1].view(torch.int16), plain[1].view(torch.int16))
        # the same windows whatever the batch size: batches of 3 reassemble to the epoch's batch of everything
        small = trainer.make_feed(DataLoader(train_ds, batch_size=3, shuffle=False), gpu_device, 0, 1)
        parts = [s.clone() for s, _ in small.batches(1, augment=True)]
        assert torch.equal(torch.cat(parts).view(torch.int32), e1[0].view(torch.int32))
        # test_model on the checkpoint, switches still on: evaluation never augments -> same loss as with the switches off
        results_on = trainer.test_model(test_loader=test_loader, model_path=cfg.CHECKPOINT_PATH / "best_model.pth",
                                        device=gpu_device, num_visualizations=1, save_visualizations=False)
        class_config.AUGMENT_SPATIAL, class_config.AUGMENT_TIME_MASKS, class_config.AUGMENT_FREQ_MASKS = False, 0, 0
        results_off = trainer.test_model(test_loader=test_loader, model_path=cfg.CHECKPOINT_PATH / "best_model.pth",
                                         device=gpu_device, num_visualizations=1, save_visualizations=False)
        assert results_on["test_loss"] == results_off["test_loss"]
    finally:
        torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = saved_det
        for k, v in saved.items():
            setattr(cfg, k, v)
