"""GPU tests of the per-channel energy normalisation: seld_pcen against the float64 definition within
four times the float32 restatement's own error, its bit-exact properties (causality, independent clips, in place, repeatable),
level invariance, every refusal, and the dataset / training / checkpoint / inference path."""
import ctypes
import functools
import subprocess
import sys
import wave
from pathlib import Path

import numpy as np
import pytest
import torch
from torch.utils.data import DataLoader

import pcen_ref as ref
from oracle import features as ofeat
from oracle import labels as olab

pytestmark = pytest.mark.gpu

PKG = Path(__file__).resolve().parent.parent / "sound-event-localization-detection_amd"
INVALID, NOT_INITIALISED, UNSUPPORTED = -1, -3, -4


def _bits(t):
    return t.contiguous().view(torch.int32)


@functools.lru_cache(maxsize=None)
def _inputs(shape_index):
    return ref.inputs(100 + shape_index, *ref.SHAPES[shape_index])


@functools.lru_cache(maxsize=None)
def _ref64(shape_index, setting_index):
    tau, alpha, delta, r, eps = ref.SETTINGS[setting_index]
    return ref.ref64(_inputs(shape_index), ref.SHAPES[shape_index][2], np.float32(ref.coefficient(tau)), alpha, delta, r, eps)


def _args(setting_index):
    import seld_native
    tau, alpha, delta, r, eps = ref.SETTINGS[setting_index]
    return (seld_native.pcen_coefficient(tau), alpha, delta, r, eps)


# ------------------------------------------------------------------------------------------------ the kernel

@pytest.mark.parametrize("setting_index", range(len(ref.SETTINGS)))
@pytest.mark.parametrize("shape_index", range(len(ref.SHAPES)))
def test_matches_the_float64_definition(gpu_device, shape_index, setting_index):
    """|y - y64| <= 4 k (delta^r + |y64|), k the float32 restatement's own factor for the setting (pcen_ref.REF32_K)."""
    import seld_native
    N, T, c_log, c_total = ref.SHAPES[shape_index]
    _, _, delta, r, _ = ref.SETTINGS[setting_index]
    x = torch.from_numpy(_inputs(shape_index)).to(gpu_device)
    assert np.float32(seld_native.pcen_coefficient(ref.SETTINGS[setting_index][0])) == np.float32(ref.coefficient(ref.SETTINGS[setting_index][0]))
    y = seld_native.pcen(x, c_log, *_args(setting_index))
    assert y.shape == x.shape and y.data_ptr() != x.data_ptr()
    assert torch.equal(_bits(y[:, :, c_log:]), _bits(x[:, :, c_log:]))          # out=None: the other channels are copies
    k = ref.error_factor(y[:, :, :c_log].cpu().numpy(), _ref64(shape_index, setting_index), delta, r)
    print(f"shape {ref.SHAPES[shape_index]} setting {ref.SETTINGS[setting_index]}: device k = {k:.3e} "
          f"(allowed {ref.DEVICE_FACTOR * ref.REF32_K[setting_index]:.1e})")
    assert k <= ref.DEVICE_FACTOR * ref.REF32_K[setting_index]


def test_causal_bit_for_bit(gpu_device):
    """The first T' frames of a run over T = 1300 equal a run over T' alone: a frame depends on nothing after it, not on
    how many chunks the clip has, and not on the ragged extent of the last one."""
    import seld_native
    x = torch.from_numpy(ref.inputs(31, 1, 1300, 4, 7)).to(gpu_device)
    for setting_index in (0, 3):
        full = seld_native.pcen(x, 4, *_args(setting_index))
        for t in (1, 256, 257, 1024):
            part = seld_native.pcen(x[:, :t].contiguous(), 4, *_args(setting_index))
            assert torch.equal(_bits(part), _bits(full[:, :t])), (setting_index, t)


def test_clips_are_independent_bit_for_bit(gpu_device):
    import seld_native
    x = torch.from_numpy(_inputs(3)).to(gpu_device)                              # (3, 257, 4, 7)
    together = seld_native.pcen(x, 4, *_args(1))
    for n in range(3):
        alone = seld_native.pcen(x[n:n + 1].contiguous(), 4, *_args(1))
        assert torch.equal(_bits(alone[0]), _bits(together[n])), n
        assert torch.equal(_bits(seld_native.pcen(x[n].contiguous(), 4, *_args(1))), _bits(together[n])), n   # [T, C, 64]
    assert not torch.equal(together[0, :, :4], together[1, :, :4])


@pytest.mark.parametrize("shape_index", [1, 3, 4])
def test_in_place_equals_out_of_place_and_other_channels_stay(gpu_device, shape_index):
    import seld_native
    N, T, c_log, c_total = ref.SHAPES[shape_index]
    x = torch.from_numpy(_inputs(shape_index)).to(gpu_device)
    keep = x.clone()
    out = torch.full_like(x, float("nan"))
    assert seld_native.pcen(x, c_log, *_args(0), out=out) is out
    assert torch.equal(_bits(x), _bits(keep))                                     # out of place: x is only read
    assert torch.isnan(out[:, :, c_log:]).all() and torch.isfinite(out[:, :, :c_log]).all()   # the NaN stays where it was
    again = torch.full_like(x, float("nan"))
    seld_native.pcen(x, c_log, *_args(0), out=again)
    assert torch.equal(_bits(again[:, :, :c_log]), _bits(out[:, :, :c_log]))      # two calls are bit-identical
    assert seld_native.pcen(x, c_log, *_args(0), out=x) is x                     # in place
    assert torch.equal(_bits(x[:, :, :c_log]), _bits(out[:, :, :c_log]))
    assert torch.equal(_bits(x[:, :, c_log:]), _bits(keep[:, :, c_log:]))
    assert not torch.equal(x[:, :, :c_log], keep[:, :, :c_log])


def test_level_invariance(gpu_device):
    """alpha = 1 and a negligible eps: y depends on E / M only, so x and x + 20 dB give the same y.  Both runs are within
    4 k (delta^r + |y64|) of their float64 results (k: the float32 restatement's own factor at this setting and input,
    measured here on the CPU), and those agree to 1e-9, so the runs agree within twice that bound.  With alpha = 0.98 a
    factor 100^0.02 = 1.10 of the level remains."""
    import seld_native
    tau, delta, r, eps = 0.4, 2.0, 0.5, 1e-20
    s = seld_native.pcen_coefficient(tau)
    x = ref.lattice_inputs(5, 1, 300, 4, 7)
    louder = x.copy()
    louder[:, :, :4] += np.float32(20.0)
    assert np.array_equal(louder[:, :, :4].astype(np.float64), x[:, :, :4].astype(np.float64) + 20.0)   # the shift is exact
    y64 = ref.ref64(x, 4, np.float32(s), 1.0, delta, r, eps)
    assert ref.error_factor(ref.ref64(louder, 4, np.float32(s), 1.0, delta, r, eps), y64, delta, r) <= 1e-9
    k = max(ref.error_factor(ref.ref32(v, 4, np.float32(s), 1.0, delta, r, eps), y64, delta, r) for v in (x, louder))
    assert k <= 4.0e-6
    xd, ld = torch.from_numpy(x).to(gpu_device), torch.from_numpy(louder).to(gpu_device)
    y = seld_native.pcen(xd, 4, s, 1.0, delta, r, eps)[:, :, :4].cpu().numpy()
    yl = seld_native.pcen(ld, 4, s, 1.0, delta, r, eps)[:, :, :4].cpu().numpy()
    for got in (y, yl):
        assert ref.error_factor(got, y64, delta, r) <= ref.DEVICE_FACTOR * k
    gap = ref.error_factor(yl, y.astype(np.float64), delta, r)
    print(f"level invariance: ref32 k = {k:.3e}, device gap = {gap:.3e}")
    assert (np.abs(yl.astype(np.float64) - y) <= 2 * ref.DEVICE_FACTOR * k * (delta ** r + np.abs(y64))).all()
    z = seld_native.pcen(xd, 4, s, 0.98, delta, r, eps)[:, :, :4].cpu().numpy()
    zl = seld_native.pcen(ld, 4, s, 0.98, delta, r, eps)[:, :, :4].cpu().numpy()
    assert ref.error_factor(zl, z.astype(np.float64), delta, r) > 1e-3


def test_refusals(gpu_device):
    """Everything include/seld_hip.h says is refused is refused with its code and a message, before any launch; the same
    arguments, unchanged, then run."""
    import seld_native
    seld_native.ensure_init(gpu_device)
    lib = seld_native.load_library()
    N, T, c_total, c_log = 2, 300, 7, 4
    x = torch.from_numpy(ref.inputs(9, N, T, c_log, c_total)).to(gpu_device)
    sentinel = -12345.0
    out = torch.full_like(x, sentinel)
    nbytes = int(lib.seld_pcen_workspace(N, T, c_total, c_log))
    assert nbytes == N * 2 * c_log * 256
    ws = torch.empty(nbytes, dtype=torch.uint8, device=gpu_device)
    good = dict(x=x.data_ptr(), out=out.data_ptr(), N=N, T=T, C_total=c_total, C_log=c_log, s=0.05, alpha=0.98, delta=2.0,
                r=0.5, eps=1e-6, ws=ws.data_ptr(), ws_bytes=nbytes)

    def call(**kw):
        a = dict(good, **kw)
        return lib.seld_pcen(a["x"], a["out"], a["N"], a["T"], a["C_total"], a["C_log"], a["s"], a["alpha"], a["delta"],
                             a["r"], a["eps"], a["ws"], a["ws_bytes"], seld_native._stream_ptr(gpu_device))
    nan, inf = float("nan"), float("inf")
    cases = [("null x", dict(x=None)), ("null out", dict(out=None)), ("null workspace", dict(ws=None)),
             ("no frames", dict(T=0)), ("negative frames", dict(T=-1)), ("no clips", dict(N=0)),
             ("no log-mel channels", dict(C_log=0)), ("more log-mel channels than channels", dict(C_log=8)),
             ("s = 0", dict(s=0.0)), ("s < 0", dict(s=-0.1)), ("s > 1", dict(s=1.5)),
             ("alpha < 0", dict(alpha=-0.1)), ("alpha > 1", dict(alpha=1.1)), ("r = 0", dict(r=0.0)), ("r > 1", dict(r=1.1)),
             ("delta = 0", dict(delta=0.0)), ("delta < 0", dict(delta=-1.0)), ("eps = 0", dict(eps=0.0)), ("eps < 0", dict(eps=-1e-6)),
             ("workspace one byte short", dict(ws_bytes=nbytes - 1)),
             ("out overlaps x", dict(out=x.data_ptr() + c_total * 256))]
    for name in ("s", "alpha", "delta", "r", "eps"):
        cases += [(f"{name} NaN", {name: nan}), (f"{name} inf", {name: inf})]
    for name, kw in cases:
        assert call(**kw) == INVALID, name
        assert lib.seld_last_error().decode().startswith("seld_pcen"), name
    assert call(x=x.data_ptr() + 4) == UNSUPPORTED and call(T=1 << 31) == UNSUPPORTED
    for bad in ((0, T, c_total, c_log), (N, 0, c_total, c_log), (N, T, c_total, 0), (N, T, c_total, 8), (N, 1 << 31, c_total, c_log)):
        assert lib.seld_pcen_workspace(*bad) == 0, bad
    torch.cuda.synchronize()
    assert (out == sentinel).all()
    assert call() == 0                                                     # and the same arguments, unchanged, run
    torch.cuda.synchronize()
    assert not (out[:, :, :c_log] == sentinel).any() and (out[:, :, c_log:] == sentinel).all()
    # the closed ends of the ranges are taken: s = 1 (M = E), alpha = 0 and 1, r = 1
    for kw in (dict(s=1.0), dict(alpha=0.0), dict(alpha=1.0), dict(r=1.0)):
        assert call(**kw) == 0, kw
    e = np.exp2(x[:, :, :c_log].cpu().numpy().astype(np.float64) * (np.log2(10.0) / 10.0))
    assert call(s=1.0, alpha=1.0, eps=1e-20) == 0                          # y = (E / E + 2)^0.5 - 2^0.5 for every element
    torch.cuda.synchronize()
    want = (e / (np.float64(np.float32(1e-20)) + e) + 2.0) ** 0.5 - 2.0 ** 0.5
    assert ref.error_factor(out[:, :, :c_log].cpu().numpy(), want, 2.0, 0.5) <= 1e-6
    # an uninitialised process gets -3 before any argument is looked at (a bare ctypes process: no torch, no seld_init)
    code = ("import ctypes, sys; lib = ctypes.CDLL(sys.argv[1]); f = ctypes.c_float; "
            "lib.seld_pcen.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_int, "
            "ctypes.c_int, f, f, f, f, f, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p]; "
            "print(lib.seld_pcen(None, None, 0, 0, 0, 0, 0, 0, 0, 0, 0, None, 0, None))")
    run = subprocess.run([sys.executable, "-c", code, str(PKG / "libseld_hip.so")], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr[-2000:]
    assert int(run.stdout.strip()) == NOT_INITIALISED
    # the binding's own checks
    with pytest.raises(seld_native.SeldNativeError, match="pcen"):
        seld_native.pcen(x.cpu(), 4, 0.05, 0.98, 2.0, 0.5, 1e-6)
    with pytest.raises(seld_native.SeldNativeError, match="seld_pcen"):
        seld_native.pcen(x, 8, 0.05, 0.98, 2.0, 0.5, 1e-6)
    with pytest.raises(seld_native.SeldNativeError, match="out"):
        seld_native.pcen(x, 4, 0.05, 0.98, 2.0, 0.5, 1e-6, out=out[:, :10])


# ------------------------------------------------------------------------------------------------ dataset and training path

class _Switches:
    """Sets a switch on the Config class and on every instance (dataset.py and trainer.py each hold one) that shadows it;
    everything is put back."""

    def __init__(self, holders):
        object.__setattr__(self, "_holders", holders)
        object.__setattr__(self, "_saved", [])

    def __setattr__(self, name, value):
        for holder in self._holders:
            if isinstance(holder, type) or name in vars(holder):
                self._saved.append((holder, name, getattr(holder, name)))
                setattr(holder, name, value)

    def restore(self):
        for holder, name, value in reversed(self._saved):
            setattr(holder, name, value)


def _clips():
    """Two FOA noise clips of different length and level, with some coherence so the intensity vectors are not ~0."""
    clips, rows = [], []
    for n in range(2):
        pcm = ofeat.synth_pcm(70 + n, 4, 24000 * (6 + 2 * n) + 977 * n, "noise") * (0.05, 1.0)[n]
        pcm[1] = 0.6 * pcm[0] + 0.4 * pcm[1]
        pcm[3] = -0.5 * pcm[0] + 0.5 * pcm[3]
        clips.append(pcm)
        rows.append(olab.synth_metadata(70 + n, meta_frames=60 + 20 * n))
    return clips, rows


@pytest.fixture
def pcen_config(gpu_device, tmp_path):
    import dataset
    import trainer
    from config import Config
    switches = _Switches((Config, dataset.config, trainer.config))
    cfg = trainer.config
    names = ("MODEL_TYPE", "CRNN_CNN_CHANNELS", "CRNN_RNN_HIDDEN", "CRNN_DROPOUT", "NUM_EPOCHS", "BATCH_SIZE", "SEED",
             "OUTPUT_PATH", "CHECKPOINT_PATH", "GRAPH_STEP", "DEVICE_FEED")
    saved = {k: getattr(cfg, k) for k in names}
    own = set(vars(cfg))
    cfg.MODEL_TYPE, cfg.CRNN_CNN_CHANNELS, cfg.CRNN_RNN_HIDDEN, cfg.CRNN_DROPOUT = "crnn", [8, 8, 16, 16], 16, 0.0
    cfg.NUM_EPOCHS, cfg.BATCH_SIZE, cfg.SEED, cfg.GRAPH_STEP, cfg.DEVICE_FEED = 1, 4, 11, True, True
    cfg.OUTPUT_PATH, cfg.CHECKPOINT_PATH = tmp_path / "outputs", tmp_path / "checkpoints"
    cfg.OUTPUT_PATH.mkdir()
    cfg.CHECKPOINT_PATH.mkdir()
    switches.FEATURE_SET = "logmel_iv"
    yield cfg, switches
    switches.restore()
    for k, v in saved.items():
        setattr(cfg, k, v)
    for name in trainer.PCEN_SETTINGS:                                     # checkpoint_payload pins them on the instance
        if name not in own and name in vars(cfg):
            delattr(cfg, name)


def test_dataset_applies_it_per_recording(gpu_device, pcen_config):
    """SELDDataset.from_pcm with the switch on: channels 0-3 of each recording's span are seld_native.pcen of the switch-off
    dataset's span, bit for bit (the stage runs before the crop: causality makes the prefix the same bits); channels 4-6 are
    the switch-off dataset's; the smoother restarts with every recording."""
    import dataset
    import seld_native
    cfg, switches = pcen_config
    clips, rows = _clips()
    off = dataset.SELDDataset.from_pcm(clips, rows, device=gpu_device)
    assert off.pcen_settings is None and off.n_channels == 7
    switches.PCEN = True
    on = dataset.SELDDataset.from_pcm(clips, rows, device=gpu_device)
    assert on.pcen_settings == {"PCEN_TIME_CONSTANT": 0.4, "PCEN_GAIN": 0.98, "PCEN_BIAS": 2.0, "PCEN_POWER": 0.5, "PCEN_EPS": 1e-10}
    assert np.array_equal(on.segments, off.segments) and len(on.segments) == 2 and on.segments[0][1] != on.segments[1][1]
    s = seld_native.pcen_coefficient(0.4)
    for start, count in ((int(a), int(b)) for a, b in on.segments):
        span = off.spec_tm[start:start + count].contiguous()
        want = seld_native.pcen(span, 4, s, 0.98, 2.0, 0.5, 1e-10)
        assert torch.equal(_bits(on.spec_tm[start:start + count, :4]), _bits(want[:, :4])), start
        assert torch.equal(_bits(on.spec_tm[start:start + count, 4:]), _bits(off.spec_tm[start:start + count, 4:])), start
    assert torch.equal(on.mask_tm, off.mask_tm) and on.rot_tm is None
    # the second recording's first frame has M = E: y = (E (eps + E)^-alpha + delta)^r - delta^r of that frame alone
    start = int(on.segments[1][0])
    e = np.exp2(off.spec_tm[start, :4].cpu().numpy().astype(np.float64) * (np.log2(10.0) / 10.0))
    alpha, eps = float(np.float32(0.98)), float(np.float32(1e-10))
    first = (e * (eps + e) ** -alpha + 2.0) ** 0.5 - 2.0 ** 0.5
    assert ref.error_factor(on.spec_tm[start, :4].cpu().numpy(), first, 2.0, 0.5) <= ref.DEVICE_FACTOR * ref.REF32_K[1]
    # ... which a smoother carried over from the first recording (20 times quieter) would not give
    carried = seld_native.pcen(off.spec_tm.contiguous(), 4, s, 0.98, 2.0, 0.5, 1e-10)
    assert ref.error_factor(carried[start, :4].cpu().numpy(), first, 2.0, 0.5) > 1e-2
    # a window of the feed is a slice of that timeline; the host mirror holds the same values
    spec, _ = on.device_batch([0, 1])
    assert torch.equal(spec[0], on.spec_tm[:on.window_length_frames])
    assert torch.equal(on[0][0], on.spec_tm[:on.window_length_frames].cpu())

    # the switches defined on dB or power values are refused before any launch: at construction and when a feed is built
    import trainer
    switches.AUGMENT_ROTATE = True
    with pytest.raises(ValueError, match="AUGMENT_ROTATE.*PCEN"):
        dataset.SELDDataset.from_pcm(clips, rows, device=gpu_device)
    switches.AUGMENT_ROTATE = False
    loader = DataLoader(on, batch_size=4, shuffle=True)
    switches.AUGMENT_MIX_PROB = 0.5
    with pytest.raises(ValueError, match="AUGMENT_MIX_PROB.*PCEN"):
        trainer.make_feed(loader, gpu_device, 0, 1)
    switches.PCEN = False                                                  # the dataset still holds PCEN values
    with pytest.raises(ValueError, match="AUGMENT_MIX_PROB.*PCEN"):
        trainer.make_feed(loader, gpu_device, 0, 1)
    switches.AUGMENT_MIX_PROB = 0.0
    switches.PCEN = True
    switches.AUGMENT_SPATIAL = True                                        # channel swaps stay allowed
    assert isinstance(trainer.make_feed(loader, gpu_device, 0, 1), trainer.DeviceFeed)
    switches.AUGMENT_SPATIAL = False
    cfg.DEVICE_FEED = False                                                # the host path refuses the switch
    with pytest.raises(RuntimeError, match="PCEN"):
        trainer.make_feed(loader, gpu_device, 0, 1)


def test_captured_training_step_on_pcen_features(gpu_device, pcen_config):
    """A captured training step with channel swaps and masks drawn reads PCEN features and gives a finite loss."""
    import dataset
    import loss as loss_mod
    import seld_graph
    import trainer
    cfg, switches = pcen_config
    switches.PCEN = True
    clips, rows = _clips()
    ds = dataset.SELDDataset.from_pcm(clips, rows, device=gpu_device)
    switches.AUGMENT_SPATIAL = True
    switches.AUGMENT_TIME_MASKS, switches.AUGMENT_TIME_MASK_MAX = 2, 40
    switches.AUGMENT_FREQ_MASKS, switches.AUGMENT_FREQ_MASK_MAX = 2, 12
    torch.manual_seed(0)
    model = trainer.prepare_model_for_device(trainer.build_model((ds.I, ds.J), True, n_channels=7), gpu_device).train()
    trainer.enable_master_weights(model, gpu_device)
    crit = loss_mod.SMRSELDLoss(loss_type=cfg.LOSS_TYPE, w_class=cfg.W_CLASS, w_aiur=cfg.W_AIUR, w_cl=cfg.W_CL,
                                grid_size=(ds.I, ds.J))
    opt = trainer.make_optimizer(model, 1e-3, gpu_device, capturable=True)
    step = trainer.make_stepper(model, crit, opt, gpu_device)
    assert isinstance(step, seld_graph.GraphedTrainStep)
    try:
        feed = trainer.make_feed(DataLoader(ds, batch_size=4, shuffle=False), gpu_device, 0, 1)
        assert isinstance(feed, trainer.DeviceFeed)
        last = None
        for _ in range(seld_graph.WARMUP + 1):                            # eager warm-up calls, then the capture
            last = next(iter(feed.batches(1, out=step.static_inputs, augment=True)))
            total, _ = step(*last)
        static = step.static_inputs(tuple(last[0].shape), last[0].dtype, tuple(last[1].shape), last[1].dtype)
        assert static is not None and step.stats()["capture_error"] is None
        spec, labels = next(iter(feed.batches(1, out=step.static_inputs, augment=True)))
        assert spec.data_ptr() == static[0].data_ptr()
        total, _ = step(spec, labels)
        assert np.isfinite(total.item())
        # PCEN values are not negative beyond the rounding of delta^r; masks were drawn
        assert (spec[:, :, :4] >= -1e-6).all() and (spec == 0).any()
    finally:
        step.close()


def test_settings_travel_through_checkpoint_inference_and_evaluation(gpu_device, pcen_config, tmp_path, monkeypatch):
    import dataset
    import infer
    import seld_native
    import trainer
    from config import Config
    from utils import safe_torch_load
    cfg, switches = pcen_config
    cfg.GRAPH_STEP = False                                                 # (the captured step has its own test above)
    clips, rows = _clips()
    switches.PCEN = True
    switches.PCEN_TIME_CONSTANT, switches.PCEN_GAIN, switches.PCEN_EPS = 0.2, 0.9, 1e-8
    settings = {"PCEN_TIME_CONSTANT": 0.2, "PCEN_GAIN": 0.9, "PCEN_BIAS": 2.0, "PCEN_POWER": 0.5, "PCEN_EPS": 1e-8}
    train_ds = dataset.SELDDataset.from_pcm(clips, rows, device=gpu_device)
    test_ds = dataset.SELDDataset.from_pcm(clips[:1], rows[:1], device=gpu_device)
    assert train_ds.pcen_settings == settings
    train_loader = DataLoader(train_ds, batch_size=cfg.BATCH_SIZE, shuffle=True)
    test_loader = DataLoader(test_ds, batch_size=cfg.BATCH_SIZE, shuffle=False)
    _, history = trainer.train_model(train_loader=train_loader, test_loader=test_loader, device=gpu_device)
    assert history["config"]["batch_source"] == "DeviceFeed"
    assert np.isfinite(history["train_losses"]).all() and np.isfinite(history["test_losses"]).all()
    best = cfg.CHECKPOINT_PATH / "best_model.pth"
    checkpoint = safe_torch_load(best, map_location="cpu")
    assert {k: vars(checkpoint["config"])[k] for k in trainer.PCEN_SETTINGS} == dict(settings, PCEN=True)
    assert trainer.checkpoint_pcen_settings(checkpoint) == settings

    # evaluation: a dataset built with the checkpoint's settings passes; any other raises, naming both sides
    result = trainer.evaluate_seld(test_loader, model_path=best, device=gpu_device)
    assert "F20" in result
    switches.PCEN_GAIN = 0.98
    other = dataset.SELDDataset.from_pcm(clips[:1], rows[:1], device=gpu_device)
    with pytest.raises(ValueError, match=r"built with PCEN on with .*PCEN_GAIN = 0.98.*checkpoint records with PCEN on with .*PCEN_GAIN = 0.9"):
        trainer.evaluate_seld(DataLoader(other, batch_size=4), model_path=best, device=gpu_device)
    switches.restore()                                                     # Config as a fresh process has it: PCEN off
    for name in trainer.PCEN_SETTINGS:
        if name in vars(trainer.config):
            delattr(trainer.config, name)
    assert Config.PCEN is False and dataset.config.PCEN is False and trainer.config.PCEN is False
    switches.FEATURE_SET = "logmel_iv"
    plain = dataset.SELDDataset.from_pcm(clips[:1], rows[:1], device=gpu_device)
    with pytest.raises(ValueError, match=r"built with PCEN off, the checkpoint records with PCEN on"):
        trainer.evaluate_seld(DataLoader(plain, batch_size=4), model_path=best, device=gpu_device)
    with pytest.raises(ValueError, match=r"built with PCEN off, the checkpoint records with PCEN on"):
        trainer.test_model(test_loader=DataLoader(plain, batch_size=4), model_path=best, device=gpu_device,
                           num_visualizations=0, save_visualizations=False)

    # infer.py builds the recording's dataset with the checkpoint's settings and leaves Config as it found it
    wav = tmp_path / "foa.wav"
    with wave.open(str(wav), "wb") as wf:
        wf.setnchannels(4)
        wf.setsampwidth(2)
        wf.setframerate(24000)
        wf.writeframes(np.ascontiguousarray(ofeat.pcm_to_int16(clips[0]).numpy().T).astype("<i2").tobytes())
    seen = []
    real = seld_native.pcen

    def spy(features, c_log, *args, **kw):
        seen.append((int(c_log),) + tuple(float(v) for v in args))
        return real(features, c_log, *args, **kw)
    monkeypatch.setattr(seld_native, "pcen", spy)
    def pcen_state():                                          # what the class says and what each instance shadows
        return ({k: getattr(Config, k) for k in trainer.PCEN_SETTINGS},
                [{k: v for k, v in vars(holder).items() if k.startswith("PCEN")} for holder in (dataset.config, trainer.config)])
    before = pcen_state()
    assert before[1] == [{}, {}]
    written = infer.main(["--checkpoint", str(best), "--out-dir", str(tmp_path / "events"), "--batch-size", "2",
                          "--threshold", "0.05", "--device", str(gpu_device), str(wav)])
    assert seen == [(4, seld_native.pcen_coefficient(0.2), 0.9, 2.0, 0.5, 1e-8)]
    assert pcen_state() == before
    assert dataset.config.PCEN is False and dataset.config.PCEN_GAIN == 0.98
    assert Path(written[0]).name == "foa.csv" and Path(written[0]).exists()
