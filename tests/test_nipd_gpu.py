"""GPU tests of the mel-band NIPD feature (csrc/nipd.hip): the kernel against the float64
restatement on the device's own phasor words, silent bins, output strides, the feature set end to end from PCM, the entry
point's refusals, and the dataset / training / inference path with FEATURE_SET = 'logmel_nipd'.

The table holds 48 taps per band, not the issue's 24 (the filterbank's widest band has 44 non-zero bins: see
tests/test_nipd_cpu.py); the tap-count refusal is therefore checked at 49.

Measured on an MI355X (max |difference| to the float64 restatement; the bars are the issue's):
  kernel on the device's own words, the 18 cases: 2.4e-8 .. 7.9e-7 m (bar 1e-5; values reach 3.43 m at 50 Hz, 5.6 m at 25 Hz)
  end to end from PCM, inner frames: float32 input 3.34e-5 m, int16 input 2.98e-5 m (bar 1e-4) -- the Q15 rounding of the
  phasor words alone gives 3.34e-5 and 3.07e-5 on these inputs, so the device's fp32 transform adds nothing that shows."""
import ctypes
import wave
from pathlib import Path

import numpy as np
import pytest
import torch

import nipd_ref as ref
from oracle import features as ofeat
from oracle import labels as olab

pytestmark = pytest.mark.gpu

RANGES = [(50.0, 2000.0), (25.0, 12000.0), (500.0, 525.0)]
SPEED = 343.0
SENTINEL = -12345.0


@pytest.fixture(scope="module")
def fb():
    return ref.library_filterbank()


def _phasor_pass(pcm):
    """seld_logmel_phasors_* on pcm [N, C, L] (device): (log-mel [N, F, C, 64], words int32 [N, C, F, pitch]).  The word
    buffer starts out as all ones, so the seven words past bin 480 of a row hold (-1, -1)."""
    import seld_native
    lib = seld_native.load_library()
    n, c, length = pcm.shape
    index = seld_native.ensure_init(pcm.device)
    frames = seld_native.num_frames(length)
    out = torch.empty((n, frames, c, 64), dtype=torch.float32, device=pcm.device)
    words = torch.full((n, c, frames, int(lib.seld_phasor_pitch())), -1, dtype=torch.int32, device=pcm.device)
    fn = lib.seld_logmel_phasors_f32 if pcm.dtype == torch.float32 else lib.seld_logmel_phasors_i16
    with torch.cuda.device(index):
        seld_native.check(fn(seld_native._p(pcm), n, c, length, seld_native._p(out), frames * c * 64, 64, 1, c * 64,
                             seld_native._p(words), seld_native._stream_ptr(pcm.device)), "seld_logmel_phasors")
    return out, words


def _noise(n, c, length, seed):
    return torch.stack([ofeat.synth_pcm(seed + i, c, length, "noise") for i in range(n)])


_words_cache = {}


def _words(gpu_device, n, c, length):
    key = (n, c, length)
    if key not in _words_cache:
        _words_cache[key] = _phasor_pass(_noise(n, c, length, 300 + c).to(gpu_device))[1]
    return _words_cache[key]


@pytest.mark.parametrize("lo,hi", RANGES)
@pytest.mark.parametrize("n,length", [(2, 9600), (3, 960)])
@pytest.mark.parametrize("channels", [2, 4, 8])
def test_kernel_against_float64_on_the_device_words(gpu_device, fb, channels, n, length, lo, hi):
    """Independent noise channels: about 2 % of the bins sit near the +-pi cut, and both sides see the same integers, so
    they agree there by construction.  Values reach pi c / (2 pi 50 Hz) = 3.4 m (6.9 m at 25 Hz); fp32 atan2f and an fp32 sum
    of at most 44 terms whose weights sum to 1 stay under a few 1e-7 relative: 1e-5 m leaves a tenfold margin."""
    import seld_native
    words = _words(gpu_device, n, channels, length)
    frames = 1 + length // 480
    _, table = seld_native.nipd_table(gpu_device, lo, hi, SPEED)
    out = torch.full((n, frames, channels - 1, 64), SENTINEL, dtype=torch.float32, device=gpu_device)
    seld_native.nipd_q15(words, out, table)
    got = out.cpu().numpy().astype(np.float64)
    weights = ref.dense_weights(fb, lo, hi, SPEED)
    host = words.cpu().numpy()
    worst = 0.0
    for i in range(n):
        want = ref.nipd_from_words(host[i], weights)                       # [C - 1, F, 64]
        worst = max(worst, float(np.abs(got[i].transpose(1, 0, 2) - want).max()))
    print(f"C={channels} N={n} F={frames} range=({lo:g}, {hi:g}): max |diff| = {worst:.3e} m, max |value| = {np.abs(got).max():.3f} m")
    assert worst <= 1e-5
    empty = ~weights.any(axis=0)
    assert (got[..., empty] == 0.0).all() and not (got == SENTINEL).any() and np.abs(got).max() > 0.1


def test_silent_bins(gpu_device):
    """A silent channel's words are 0: its phase is 0 by definition, whichever side of the product it is on."""
    import seld_native
    pcm = _noise(2, 4, 9600, 410)
    _, table = seld_native.nipd_table(gpu_device, 50.0, 2000.0, SPEED)

    def run(x):
        _, words = _phasor_pass(x.to(gpu_device))
        out = torch.full((2, 21, 3, 64), SENTINEL, dtype=torch.float32, device=gpu_device)
        return seld_native.nipd_q15(words, out, table).cpu().numpy(), words
    base, _ = run(pcm)
    dead = pcm.clone()
    dead[:, 2] = 0.0
    got, words = run(dead)
    assert (words[:, 2, :, :481] == 0).all()
    assert (got[:, :, 1] == 0.0).all()                                     # nipd_2: exactly 0 everywhere
    for m in (0, 2):                                                       # the others: bit for bit what they were
        assert np.array_equal(got[:, :, m].view(np.uint32), base[:, :, m].view(np.uint32))
    dead = pcm.clone()
    dead[:, 0] = 0.0
    got, _ = run(dead)
    assert (got == 0.0).all() and (base != 0.0).any()


@pytest.mark.parametrize("channels", [3, 8])
def test_output_strides_into_the_feature_tensor(gpu_device, fb, channels):
    import seld_native
    words = _words(gpu_device, 2, channels, 9600) if channels == 8 else _phasor_pass(_noise(2, channels, 9600, 77).to(gpu_device))[1]
    _, table = seld_native.nipd_table(gpu_device, 50.0, 2000.0, SPEED)
    dense = torch.full((2, 21, channels - 1, 64), SENTINEL, dtype=torch.float32, device=gpu_device)
    seld_native.nipd_q15(words, dense, table)
    feat = torch.full((2, 21, 2 * channels - 1, 64), SENTINEL, dtype=torch.float32, device=gpu_device)
    seld_native.nipd_q15(words, feat[:, :, channels:], table)
    assert (feat[:, :, :channels] == SENTINEL).all()                       # the log-mel channels keep the sentinel,
    assert not (feat[:, :, channels:] == SENTINEL).any()                   # nothing else does,
    assert torch.equal(feat[:, :, channels:], dense)                       # and the values do not depend on the strides
    empty = torch.from_numpy(~ref.dense_weights(fb, 50.0, 2000.0, SPEED).any(axis=0)).to(gpu_device)
    assert int(empty.sum()) == 33 and (feat[:, :, channels:][..., empty] == 0.0).all()


@pytest.fixture(scope="module")
def delayed():
    pcm = ref.delayed_noise()
    return pcm, ref.dense_weights(ref.library_filterbank(), 50.0, 2000.0, SPEED)


@pytest.mark.parametrize("dtype", ["float32", "int16"])
def test_feature_set_from_pcm(gpu_device, delayed, dtype):
    """'logmel_nipd' end to end on the delayed-noise input of the CPU test: the log-mel channels are those of 'logmel_gcc'
    bit for bit, the NIPD channels agree with the float64 restatement from PCM to the 1e-4 m that tests/test_spatial_gpu.py
    holds the spatial features to, and their median reads c d / 24000 within 1 %."""
    import seld_native
    pcm, weights = delayed
    x = torch.from_numpy(pcm)
    if dtype == "int16":
        x = ofeat.pcm_to_int16(x)
        pcm = ofeat.int16_to_pcm(x).numpy()
    feat = seld_native.spatial_features(x.to(gpu_device), "logmel_nipd")
    assert tuple(feat.shape) == (21, 15, 64)
    gcc = seld_native.spatial_features(x.to(gpu_device), "logmel_gcc")
    assert torch.equal(feat[:, :8].view(torch.int32), gcc[:, :8].view(torch.int32))
    got = feat[:, 8:].cpu().numpy().astype(np.float64).transpose(1, 0, 2)  # [7, F, 64]
    want = ref.nipd_from_pcm(pcm, weights)
    err = np.abs(got - want)[:, 1:-1]
    model = np.abs(ref.nipd_from_pcm(pcm, weights, q15=True) - want)[:, 1:-1].max()
    print(f"{dtype}: max |diff| to float64 from PCM on the inner frames = {err.max():.3e} m (Q15 rounding model alone: "
          f"{model:.3e} m)")
    assert err.max() <= 1e-4
    bands = np.nonzero(weights.any(axis=0))[0]
    for m, d in enumerate(ref.DELAYS[1:]):
        want_m = SPEED * d / 24000.0
        assert abs(np.median(got[m, 1:-1][:, bands]) - want_m) <= 0.01 * abs(want_m), (d, want_m)
    # the keyword arguments pick the range; the defaults are the Config values
    same = seld_native.spatial_features(x.to(gpu_device), "logmel_nipd", nipd_min_hz=50.0, nipd_max_hz=2000.0, sound_speed=343.0)
    assert torch.equal(same, feat)
    wide = seld_native.spatial_features(x.to(gpu_device), "logmel_nipd", nipd_max_hz=4000.0)
    assert int((wide[:, 8:] != 0).any(dim=0).any(dim=0).sum()) > len(bands)
    for channels in (1, 9):
        with pytest.raises(ValueError, match="2..8 channels"):
            seld_native.spatial_features(torch.zeros(channels, 960, device=gpu_device), "logmel_nipd")
    with pytest.raises(ValueError, match="unknown feature kind"):
        seld_native.spatial_features(x.to(gpu_device), "logmel_salsa")


def test_refusals(gpu_device):
    """Every refusal of seld_nipd_q15 returns its code before anything is launched: the sentinel-filled output stays."""
    import seld_native
    lib = seld_native.load_library()
    words = _words(gpu_device, 2, 4, 9600)
    (first, taps, w, _), table = seld_native.nipd_table(gpu_device, 50.0, 2000.0, SPEED)
    out = torch.full((2, 21, 3, 64), SENTINEL, dtype=torch.float32, device=gpu_device)
    stream = seld_native._stream_ptr(gpu_device)
    good = dict(phasors=words.data_ptr(), N=2, C=4, F=21, table=table.data_ptr(), out=out.data_ptr(), sN=21 * 192, sC=64,
                sM=1, sT=192)

    def call(**kw):
        a = dict(good, **kw)
        return lib.seld_nipd_q15(ctypes.c_void_p(a["phasors"]), a["N"], a["C"], a["F"], ctypes.c_void_p(a["table"]),
                                 ctypes.c_void_p(a["out"]), a["sN"], a["sC"], a["sM"], a["sT"], stream)
    too_many = taps.copy()
    too_many[5] = seld_native.NIPD_MAX_TAPS + 1
    bad_taps = seld_native.nipd_pack_table(first, too_many, w).to(gpu_device)
    negative = taps.copy()
    negative[7] = -1
    bad_negative = seld_native.nipd_pack_table(first, negative, w).to(gpu_device)
    outside = first.copy()
    outside[30] = 480
    bad_first = seld_native.nipd_pack_table(outside, taps, w).to(gpu_device)
    no_taps = seld_native.nipd_pack_table(first, np.zeros_like(taps), w).to(gpu_device)
    cases = [("null phasors", dict(phasors=None), -1), ("null table", dict(table=None), -1), ("null out", dict(out=None), -1),
             ("one channel", dict(C=1), -4), ("nine channels", dict(C=9), -4), ("no frames", dict(F=0), -1),
             ("no clips", dict(N=0), -1), ("negative clips", dict(N=-1), -1), ("band stride 2", dict(sM=2), -4),
             ("misaligned out", dict(out=out.data_ptr() + 4), -4), ("odd row stride", dict(sT=194), -4),
             ("49 taps", dict(table=bad_taps.data_ptr()), -1), ("negative taps", dict(table=bad_negative.data_ptr()), -1),
             ("band past bin 480", dict(table=bad_first.data_ptr()), -1), ("empty table", dict(table=no_taps.data_ptr()), -1)]
    for name, kw, code in cases:
        assert call(**kw) == code, name
        assert lib.seld_last_error().decode().startswith("seld_nipd_q15"), name
    torch.cuda.synchronize()
    assert (out == SENTINEL).all()
    assert call() == 0                                                     # and the same arguments, unchanged, run
    torch.cuda.synchronize()
    assert not (out == SENTINEL).any()


# ------------------------------------------------------------------------------------------------ dataset path

@pytest.fixture
def nipd_config(tmp_path):
    """FEATURE_SET = 'logmel_nipd' and a small CRNN on the Config class and on the instances dataset.py and trainer.py
    hold; everything is put back."""
    import dataset
    import trainer
    from config import Config
    holders = (Config, dataset.config, trainer.config)
    saved = []

    def put(name, value):
        for holder in holders:
            if isinstance(holder, type) or name in vars(holder):
                saved.append((holder, name, getattr(holder, name)))
                setattr(holder, name, value)
    put("FEATURE_SET", "logmel_nipd")
    put("MODEL_TYPE", "crnn")
    put("CRNN_CNN_CHANNELS", [8, 8, 16, 16])
    put("CRNN_RNN_HIDDEN", 16)
    put("CRNN_DROPOUT", 0.0)
    own = set(vars(trainer.config))
    yield put
    for holder, name, value in reversed(saved):
        setattr(holder, name, value)
    for name in trainer.NIPD_SETTINGS:                                     # checkpoint_payload pins them on the instance
        if name not in own and name in vars(trainer.config):
            delattr(trainer.config, name)


def _array_clips():
    clips, rows = [], []
    for i in range(2):
        pcm = ofeat.synth_pcm(500 + i, 8, 24000 * 6, "noise")
        pcm[3, 2:] = pcm[0, :-2]                                           # microphone 3: microphone 0 two samples later
        clips.append(pcm)
        rows.append(olab.synth_metadata(500 + i, meta_frames=60))
    return clips, rows


def test_dataset_training_and_inference_path(gpu_device, fb, nipd_config, tmp_path, monkeypatch):
    import dataset
    import infer
    import seld_augment
    import seld_native
    import trainer
    clips, rows = _array_clips()
    ds = dataset.SELDDataset.from_pcm(clips, rows, device=gpu_device)
    assert ds.n_channels == 15
    empty = torch.from_numpy(~ref.dense_weights(fb, 50.0, 2000.0, SPEED).any(axis=0)).to(gpu_device)
    live_bands = [j for j in range(64) if not bool(empty[j])]
    # the timeline is the clips' feature tensors; a gathered window is a slice of it
    for i, pcm in enumerate(clips):
        start, count = (int(v) for v in ds.segments[i])
        assert torch.equal(ds.spec_tm[start:start + count], seld_native.spatial_features(pcm.to(gpu_device), "logmel_nipd")[:count])
    w = ds.window_length_frames
    spec, mask = ds.device_batch([0, 1])
    assert tuple(spec.shape) == (2, w, 15, 64)
    for b in range(2):
        s = int(ds.window_starts[b])
        assert torch.equal(spec[b], ds.spec_tm[s:s + w])
    assert (spec[:, :, 8:][..., empty] == 0.0).all() and (spec[:, :, 8:][..., ~empty] != 0.0).any()
    # microphone 3 reads as two samples of path in the median
    lag = spec[0, 2:-2, 8 + 2][:, ~empty].median().item()
    assert abs(lag - SPEED * 2 / 24000.0) <= 0.01 * SPEED * 2 / 24000.0
    # standardised: the flat out-of-range bands are only centred and stay exactly 0
    stats = ds.feature_statistics()
    assert (stats["std"][8:][:, empty.cpu()] < 1e-6).all() and (stats["mean"][8:][:, empty.cpu()] == 0).all()
    ds.set_feature_statistics(stats)
    std_spec = ds.device_batch([0, 1])[0]
    assert (std_spec[:, :, 8:][..., empty] == 0.0).all() and not torch.equal(std_spec, spec)
    ds.set_feature_statistics(None)
    # two frequency masks reach the NIPD channels (all 2C - 1 channels lie on the mel axis)
    assert seld_augment.freq_mask_channels("logmel_nipd", ds.n_channels) == 15
    rows_aug = seld_augment.identity_rows(2)
    rows_aug[:, 5:9] = (live_bands[3], 4, live_bands[20], 5)
    masked = ds.device_batch([0, 1], augment=rows_aug)[0]
    hit = torch.zeros(64, dtype=torch.bool, device=gpu_device)
    hit[live_bands[3]:live_bands[3] + 4] = True
    hit[live_bands[20]:live_bands[20] + 5] = True
    assert (masked[..., hit] == 0.0).all() and (spec[:, :, 8:][..., hit] != 0.0).any()
    assert torch.equal(masked[..., ~hit], spec[..., ~hit])

    # one training step of the small CRNN on 15 input channels
    torch.manual_seed(0)
    model = trainer.prepare_model_for_device(trainer.build_model((ds.I, ds.J), True, n_channels=ds.n_channels), gpu_device).train()
    crit = trainer.SMRSELDLoss(loss_type="mse", w_class=1.0, grid_size=(ds.I, ds.J))
    trainer.enable_master_weights(model, gpu_device)
    opt = trainer.make_optimizer(model, 1e-3, gpu_device)
    before = [p.detach().float().clone() for p in model.parameters()]
    loss, _ = trainer.train_step(model, crit, opt, spec, mask, gpu_device)
    assert np.isfinite(loss.item())
    assert any(not torch.equal(b, p.detach().float()) for b, p in zip(before, model.parameters()))

    # a checkpoint of that model carries the NIPD settings; infer.py computes the recording's features with THEM
    # (a plumbing check: the file is made to say 1500 Hz, the process says 2000)
    trainer.config.NIPD_MAX_HZ = 1500.0
    checkpoint = tmp_path / "crnn_nipd.pth"
    torch.save(trainer.checkpoint_payload(0, model, opt, 0.0, 0.0), checkpoint)
    assert {k: vars(trainer.config)[k] for k in trainer.NIPD_SETTINGS} == \
        {"NIPD_MIN_HZ": 50.0, "NIPD_MAX_HZ": 1500.0, "SOUND_SPEED": 343.0}
    assert dataset.config.NIPD_MAX_HZ == 2000.0
    wav = tmp_path / "array.wav"
    with wave.open(str(wav), "wb") as wf:
        wf.setnchannels(8)
        wf.setsampwidth(2)
        wf.setframerate(24000)
        wf.writeframes(np.ascontiguousarray(ofeat.pcm_to_int16(clips[0]).numpy().T).astype("<i2").tobytes())
    seen = []
    real = seld_native.spatial_features

    def spy(pcm, kind, **kw):
        seen.append((kind, kw))
        return real(pcm, kind, **kw)
    monkeypatch.setattr(seld_native, "spatial_features", spy)
    written = infer.main(["--checkpoint", str(checkpoint), "--out-dir", str(tmp_path / "events"), "--batch-size", "2",
                          "--threshold", "0.05", "--device", str(gpu_device), str(wav)])
    assert seen == [("logmel_nipd", dict(nipd_min_hz=50.0, nipd_max_hz=1500.0, sound_speed=343.0))]
    assert dataset.config.NIPD_MAX_HZ == 2000.0                            # put back after the run
    assert Path(written[0]).name == "array.csv" and Path(written[0]).exists()
