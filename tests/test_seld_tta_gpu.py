"""GPU checks of test-time augmentation in the SELD evaluation (csrc/seld_tta.hip, seld_eval.grid_decode_tta / decode /
evaluate_logits with ``patterns``, trainer.timeline_logits / evaluate_seld, infer.py --tta) against the float64
restatement of DESIGN.md section 13 (tests/seld_tta_ref.py) and against the plain decode."""
import math
import subprocess
import sys
import wave
from pathlib import Path

import numpy as np
import pytest
import torch

import seld_eval_ref as ref
import seld_tta_ref as tta

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
PKG = ROOT / "sound-event-localization-detection_amd"
Q = 22


def _device_case(name, gpu_device):
    dtype, patterns, x, want = tta.case(name)
    t = torch.from_numpy(x)
    if dtype == "bf16":
        t = t.to(torch.bfloat16)                                   # exact: the values are bf16 already
    return patterns, t.to(gpu_device), want


@pytest.fixture(scope="module", params=list(tta.CASES))
def planted(request, gpu_device):
    """(case name, patterns, device logits [P, 3, 250, 648, 14], float64 reference P_q [22, 648, 13])."""
    return (request.param,) + _device_case(request.param, gpu_device)


@pytest.fixture(scope="module")
def table():
    import seld_eval
    t = seld_eval.meta_frame_table(tta.SEG, tta.TOTAL)
    assert len(t) == Q and t.windows == 3
    return t


@pytest.mark.parametrize("k", [1, 4, 8])
def test_tta_decode_matches_float64_reference(planted, table, k):
    """bf16 / all 16 patterns, fp32 / (2, 6, 11), fp32 / (3,) on a 103-frame timeline of two segments.  P_q within 2e-5
    of the float64 restatement (the bar of the plain decode: the longer sums are divided by n_w * n, so their rounding
    error shrinks with them); detections (count, cells, order) exact outside near ties, which may exclude at most 1 %
    of the 286 entries -- the restatement alone finds none, with 38 / 58 / 63, 42 / 59 / 62 and 46 / 66 / 73 detections at
    K = 1 / 4 / 8.  Un-permuting in the wrong direction would move P_q by 0.24 / 0.65 / 0.98, decoding stack 0 alone by
    0.19 / 0.14 in the first two."""
    import seld_eval
    name, patterns, logits, want = planted
    probs = torch.full((Q, 648, 13), float("nan"), dtype=torch.float32, device=logits.device)
    cells, scores, counts = seld_eval.grid_decode_tta(logits, patterns, 0, table, 0, Q, tta.THRESHOLD, k, probs=probs)
    got = probs.cpu().double().numpy()
    err = float(np.abs(got - want).max())
    print(f"{name} K={k}: max |P_q - float64| = {err:.3e}")
    assert err <= 2e-5
    ref_dets, near = ref.decode_detections(want, tta.THRESHOLD, k)
    cells, scores, counts = cells.cpu().numpy(), scores.cpu().numpy(), counts.cpu().numpy()
    share = float(near.mean())
    print(f"{name} K={k}: near-tie exclusions {int(near.sum())} of {near.size} ({100 * share:.3f} %), "
          f"{sum(len(c) for r in ref_dets for c in r)} reference detections")
    assert near.size == 286 and share <= 0.01
    mismatches = []
    for q in range(Q):
        for c in range(13):
            n = int(counts[q, c])
            assert (cells[q, c, n:] == -1).all() and (scores[q, c, n:] == 0).all()
            assert np.array_equal(scores[q, c, :n], got[q, cells[q, c, :n], c].astype(np.float32))
            if not near[q, c] and cells[q, c, :n].tolist() != ref_dets[q][c]:
                mismatches.append((q, c, cells[q, c, :n].tolist(), ref_dets[q][c]))
    assert not mismatches, mismatches[:5]


@pytest.fixture(scope="module")
def plain_base(gpu_device, table):
    """(base logits fp32 [3, 250, 648, 14] on the device, grid_decode of them at K = 4 with P_q)."""
    import seld_eval
    base = torch.from_numpy(ref.planted_logits(tta.SEG, 2234)).to(gpu_device)
    probs = torch.empty((Q, 648, 13), dtype=torch.float32, device=gpu_device)
    out = seld_eval.grid_decode(base, 0, table, 0, Q, tta.THRESHOLD, 4, probs=probs)
    assert int(out[2].sum()) > 40
    return base, (*out, probs)


@pytest.mark.parametrize("p", range(16))
def test_every_pattern_alone_is_the_plain_decode(plain_base, table, p):
    """One exact permuted copy under patterns = (p,) reads, cell for cell, what the plain kernel reads from the base in
    the same order: all four outputs are bit-identical.  p = 0: the identity equals the plain kernel."""
    import seld_augment
    import seld_eval
    base, want = plain_base
    src = torch.from_numpy(seld_augment.cell_source(p)).to(base.device)
    stack = base.index_select(2, src).unsqueeze(0)
    probs = torch.full((Q, 648, 13), float("nan"), dtype=torch.float32, device=base.device)
    got = (*seld_eval.grid_decode_tta(stack, (p,), 0, table, 0, Q, tta.THRESHOLD, 4, probs=probs), probs)
    for a, b in zip(got, want):
        assert torch.equal(a, b)


def test_launches_streaming_and_splits_are_bit_identical(gpu_device, table):
    """bf16 / all 16: one launch over everything, a second run, the streaming driver fed 2 windows at a time and
    meta-frame ranges (0, 7), (7, 8), (8, 22) give the same bits."""
    import seld_eval
    patterns, logits, _ = _device_case("bf16-all", gpu_device)

    def whole():
        probs = torch.empty((Q, 648, 13), dtype=torch.float32, device=gpu_device)
        return (*seld_eval.grid_decode_tta(logits, patterns, 0, table, 0, Q, tta.THRESHOLD, 4, probs=probs), probs)

    one = whole()
    again = whole()
    streamed = seld_eval.decode((logits[:, lo:lo + 2] for lo in range(0, 3, 2)), table, tta.THRESHOLD, 4, keep_probs=True,
                                patterns=patterns)
    split = [torch.empty_like(t) for t in one]
    for lo, hi in ((0, 7), (7, 8), (8, Q)):
        seld_eval.grid_decode_tta(logits, patterns, 0, table, lo, hi - lo, tta.THRESHOLD, 4,
                                  out=tuple(t[lo:hi] for t in split[:3]), probs=split[3][lo:hi])
    assert int(one[2].sum()) == 58
    for a, b, c, d in zip(one, again, streamed, split):
        assert torch.equal(a, b) and torch.equal(a, c) and torch.equal(a, d)


def test_error_paths(gpu_device, table):
    import seld_eval
    from seld_native import SeldNativeError
    logits = torch.zeros((2, 3, 250, 648, 14), dtype=torch.float32, device=gpu_device)

    def fresh(k=4):
        return (torch.full((Q, 13, max(k, 1)), 77, dtype=torch.int32, device=gpu_device),
                torch.full((Q, 13, max(k, 1)), 77.0, dtype=torch.float32, device=gpu_device),
                torch.full((Q, 13), 77, dtype=torch.int32, device=gpu_device))

    out = fresh()
    probs = torch.full((Q, 648, 13), 77.0, dtype=torch.float32, device=gpu_device)
    # the library's own checks of the list (the C entry point, through the binding): code -1.  One window of 50 frames,
    # so that 17 stacks stay small
    small = seld_eval.meta_frame_table(np.array([[0, 50]]))
    wide = torch.zeros((17, 1, 250, 648, 14), dtype=torch.bfloat16, device=gpu_device)
    for patterns in ((), tuple(range(16)) + (0,), (0, 16), (-1, 0), (5, 5), (0, 1, 2, 1)):
        with pytest.raises(SeldNativeError, match="code -1"):
            seld_eval.grid_decode_tta(wide[:len(patterns)], patterns, 0, small, 0, 10, 0.5, 4,
                                      out=tuple(t[:10] for t in out), probs=probs[:10])
    del wide
    for stacks, patterns in ((2, (0,)), (2, (0, 1, 2)), (1, (0, 1))):
        with pytest.raises(ValueError):
            seld_eval.grid_decode_tta(logits[:stacks], patterns, 0, table, 0, Q, 0.5, 4, out=out, probs=probs)
    with pytest.raises(ValueError):                                     # a plain [nw, 250, 648, 14] batch
        seld_eval.grid_decode_tta(logits[0], (0,), 0, table, 0, Q, 0.5, 4, out=out, probs=probs)
    for k in (0, 9):
        with pytest.raises(SeldNativeError, match="code -1"):
            seld_eval.grid_decode_tta(logits, (0, 1), 0, table, 0, Q, 0.5, k, out=fresh(k))
        with pytest.raises(ValueError):
            seld_eval.decode(iter([logits]), table, 0.5, k, patterns=(0, 1))
    # a covering window is missing: refused on the host, nothing launched
    with pytest.raises(SeldNativeError, match="need windows"):          # windows 1..2 only: meta-frame 0 needs window 0
        seld_eval.grid_decode_tta(logits[:, 1:], (0, 1), 1, table, 0, Q, 0.5, 4, out=out, probs=probs)
    with pytest.raises(SeldNativeError, match="need windows"):          # windows 0..1 only: frames 100.. need window 2
        seld_eval.grid_decode_tta(logits[:, :2], (0, 1), 0, table, 0, Q, 0.5, 4, out=out, probs=probs)
    torch.cuda.synchronize()
    assert all((t == 77).all() for t in out) and (probs == 77).all()
    ok = seld_eval.grid_decode_tta(logits, (0, 1), 0, table, 0, Q, 0.5, 4)
    assert (ok[2] == 0).all()                                            # uniform maps: no peak


def test_end_to_end_perfect_predictor_through_the_gathers(gpu_device, tmp_path):
    """Stack n = 20 x the one-hot of the labels the augmenting gather gives for pattern p_n (the labels of the
    transformed sound field), batches of 3 windows, all 16 patterns: the averaged maps are the un-permuted labels, so
    F20 = 1, ER20 = 0, LR_CD = 1, LE_CD <= 7.1, counts and LE_CD as the plain evaluation of the plain labels, and the
    CSVs rasterise to the input rows' labels."""
    import dataset
    import seld_augment
    import seld_eval
    import seld_native
    ds, rows, frames = tta.two_clip_dataset(gpu_device, 5)
    patterns = tuple(range(16))

    def batches():
        for lo in range(0, len(ds), 3):
            idx = list(range(lo, min(lo + 3, len(ds))))
            yield torch.stack([20.0 * seld_native.expand_labels(ds.device_batch(idx, augment=seld_augment.tta_rows(p, len(idx)))[1])
                               for p in patterns])

    def plain_batches():
        for lo in range(0, len(ds), 3):
            yield 20.0 * seld_native.expand_labels(ds.device_batch(list(range(lo, min(lo + 3, len(ds)))))[1])

    res = seld_eval.evaluate_logits(batches(), ds, events_dir=tmp_path, names=["first", "second"], patterns=patterns)
    plain = seld_eval.evaluate_logits(plain_batches(), ds)
    print({k: res[k] for k in ("F20", "ER20", "LE_CD", "LR_CD", "TP", "FP", "FN", "N")})
    assert res["tta_patterns"] == list(range(16)) and plain["tta_patterns"] == []
    assert res["N"] > 100
    assert res["F20"] == 1.0 and res["ER20"] == 0.0 and res["LR_CD"] == 1.0 and res["LE_CD"] <= 7.1
    for key in ("TP", "FP", "FN", "N", "LE_CD"):
        assert res[key] == plain[key], key
    for s, name in enumerate(("first", "second")):
        written = dataset._read_metadata_rows(tmp_path / f"{name}.csv")
        got = seld_native.rasterise_labels(torch.from_numpy(written), frames[s], device=gpu_device)
        want = seld_native.rasterise_labels(torch.from_numpy(rows[s]), frames[s], device=gpu_device)
        assert torch.equal(got, want)


@pytest.fixture(scope="module")
def crnn_checkpoint(gpu_device, tmp_path_factory):
    """A seeded, untrained CRNN written in the trainer's checkpoint format."""
    import trainer
    old = trainer.config.MODEL_TYPE
    trainer.config.MODEL_TYPE = "crnn"
    torch.manual_seed(0)
    model = trainer.prepare_model_for_device(trainer.build_model((18, 36), True, n_channels=4), gpu_device)
    path = tmp_path_factory.mktemp("seld_tta") / "crnn.pth"
    torch.save({"epoch": 0, "model_state_dict": trainer.model_state_dict(model), "train_loss": 0.0, "test_loss": 0.0},
               path)
    yield path
    trainer.config.MODEL_TYPE = old


def _same(a, b):
    if isinstance(a, float) and isinstance(b, float) and math.isnan(a) and math.isnan(b):
        return True
    if isinstance(a, list):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(_same(a[k], b[k]) for k in a)
    return a == b


@pytest.fixture
def deterministic_convolutions():
    """MIOpen's default convolution solutions for the CRNN's shapes are not bitwise repeatable from call to call; its
    deterministic mode is (tests/test_seld_eval_gpu.py)."""
    saved = torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark
    torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = True, False
    yield
    torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = saved


KEYS = ("F20", "ER20", "LE_CD", "LR_CD", "TP", "FP", "FN", "N", "S", "D", "I", "per_class")


def test_evaluate_seld_with_tta_equals_evaluate_logits_of_the_gathered_stacks(gpu_device, crnn_checkpoint, tmp_path,
                                                                              deterministic_convolutions):
    """Plumbing: evaluate_seld(tta=(0, 3, 10)) on the checkpoint equals evaluate_logits(patterns=(0, 3, 10)) over logits
    computed here with device_batch(..., augment=tta_rows(p, B)), exactly (the untrained model's probabilities sit near
    1/14: one differing logit bit moves detections); with TTA off, in the same process, evaluate_seld() equals the plain
    evaluate_logits; unsupported feature sets are refused when evaluation starts."""
    from torch.utils.data import DataLoader
    import seld_augment
    import seld_eval
    import trainer
    from utils import safe_torch_load
    ds, _, _ = tta.two_clip_dataset(gpu_device, 9)
    threshold = 1.0 / 14.0 + 1e-4
    patterns = (0, 3, 10)
    loader = DataLoader(ds, batch_size=3, shuffle=False)
    got = trainer.evaluate_seld(loader, model_path=crnn_checkpoint, device=gpu_device, threshold=threshold, max_peaks=8,
                                events_dir=tmp_path / "events", tta=patterns)
    got_off = trainer.evaluate_seld(loader, model_path=crnn_checkpoint, device=gpu_device, threshold=threshold, max_peaks=8)
    model = trainer.prepare_model_for_device(trainer.build_model((ds.I, ds.J), True, n_channels=ds.n_channels),
                                             gpu_device)
    model.load_state_dict(safe_torch_load(crnn_checkpoint, map_location=gpu_device)["model_state_dict"])
    model.eval()
    stacks, plain = [], []
    for lo in range(0, len(ds), 3):
        idx = list(range(lo, min(lo + 3, len(ds))))
        per_pattern = []
        for p in patterns:
            spec, _ = ds.device_batch(idx, augment=seld_augment.tta_rows(p, len(idx)))
            with torch.no_grad(), trainer.autocast_context(gpu_device):
                per_pattern.append(model(spec))
        stacks.append(torch.stack(per_pattern))
        spec, _ = ds.device_batch(idx)
        with torch.no_grad(), trainer.autocast_context(gpu_device):
            plain.append(model(spec))
    want = seld_eval.evaluate_logits(iter(stacks), ds, threshold=threshold, max_peaks=8, patterns=patterns)
    want_off = seld_eval.evaluate_logits(iter(plain), ds, threshold=threshold, max_peaks=8)
    print({k: got[k] for k in KEYS[:8]}, {k: got_off[k] for k in KEYS[:8]})
    assert got["TP"] + got["FP"] > 0 and got_off["TP"] + got_off["FP"] > 0
    for key in KEYS:
        assert _same(got[key], want[key]), key
        assert _same(got_off[key], want_off[key]), key
    assert got["tta_patterns"] == [0, 3, 10] and want["tta_patterns"] == [0, 3, 10]
    assert got_off["tta_patterns"] == [] and want_off["tta_patterns"] == []
    assert len(got["event_files"]) == 2 and got["checkpoint_epoch"] == 0
    # a microphone-array feature set has no channel swap: refused before the checkpoint is even read
    saved = ds.n_channels
    try:
        ds.n_channels = 10                                              # the shape of 'logmel_gcc' on 4 microphones
        with pytest.raises(ValueError, match="microphone array"):
            trainer.evaluate_seld(loader, model_path=crnn_checkpoint, device=gpu_device, tta="all")
    finally:
        ds.n_channels = saved
    saved = getattr(trainer.config, "FEATURE_SET", "logmel")
    try:
        trainer.config.FEATURE_SET = "logmel_gcc"
        with pytest.raises(ValueError, match="microphone array"):
            trainer.evaluate_seld(loader, model_path=crnn_checkpoint, device=gpu_device, tta="all")
        seld_augment.check_tta((), "logmel_gcc", ds.n_channels)          # (TTA off is not refused)
    finally:
        trainer.config.FEATURE_SET = saved


def test_infer_cli_with_tta_writes_event_csv(gpu_device, crnn_checkpoint, tmp_path):
    import dataset
    rng = np.random.default_rng(4)
    pcm = (rng.standard_normal((24000 * 5, 4)) * 3000).clip(-32768, 32767).astype("<i2")
    wav = tmp_path / "synthetic_take.wav"
    with wave.open(str(wav), "wb") as wf:
        wf.setnchannels(4)
        wf.setsampwidth(2)
        wf.setframerate(24000)
        wf.writeframes(pcm.tobytes())
    out = tmp_path / "events"
    run = subprocess.run([sys.executable, str(PKG / "infer.py"), "--checkpoint", str(crnn_checkpoint), "--out-dir", str(out),
                          "--model-type", "crnn", "--threshold", str(1.0 / 14.0 + 1e-4), "--max-peaks", "8", "--tta", "0,3",
                          str(wav)], capture_output=True, text=True, timeout=600, cwd=str(ROOT))
    print(run.stdout[-2000:], run.stderr[-4000:])
    assert run.returncode == 0
    rows = dataset._read_metadata_rows(out / "synthetic_take.csv")
    assert rows.shape[1] == 5 and rows.shape[0] > 0
    assert ((rows[:, 1] >= 0) & (rows[:, 1] < 13)).all() and ((rows[:, 2] >= 0) & (rows[:, 2] < 8)).all()
    assert rows[:, 0].max() < 50                                   # 5 s = 250 frames = 50 meta-frames
