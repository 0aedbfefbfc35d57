"""GPU checks of the SELD evaluation path (csrc/seld_eval.hip, seld_eval.py, trainer.evaluate_seld, infer.py) against the
float64 restatement of DESIGN.md section 10 (tests/seld_eval_ref.py)."""
import math
import subprocess
import sys
import wave
from pathlib import Path

import numpy as np
import pytest
import torch

import seld_eval_ref as ref

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
PKG = ROOT / "sound-event-localization-detection_amd"
SEGMENTS = np.array([[0, 503], [503, 250], [753, 1001]])      # tail windows, windows across segments, partial meta-frames
TOTAL = 1754
THRESHOLD = 0.5
SEEDS = {"fp32": 1234, "bf16": 1235}


@pytest.fixture(scope="module", params=["fp32", "bf16"])
def planted(request, gpu_device):
    """(dtype name, device logits [36, 250, 648, 14], float64 reference P_q [Q, 648, 13])."""
    x = ref.planted_logits(SEGMENTS, SEEDS[request.param])
    t = torch.from_numpy(x)
    if request.param == "bf16":
        t = t.to(torch.bfloat16)
        x = t.float().numpy()                                       # the bf16 inputs, upcast exactly
    probs = ref.decode_probs(x, SEGMENTS, TOTAL)
    return request.param, t.to(gpu_device), probs


@pytest.mark.parametrize("k", [1, 4, 8])
def test_decode_matches_float64_reference(planted, k):
    """Planted-peak logits, 3 segments (503, 250, 1001 frames), bf16 and fp32.  P_q within 2e-5 of the float64
    restatement; detections (count, cells, order) exact outside near ties, which are at most 1 % of the entries.
    Measured with the restatement alone on the CPU for these seeds and this layout (threshold 0.5): fp32 / seed 1234
    excludes 1 of 4 576 entries (0.022 %) for K = 1, 4, 8 with 564 / 838 / 899 detections; bf16 / seed 1235 excludes
    5 of 4 576 (0.109 %) with 602 / 865 / 914 detections; K = 1 and 4 truncate (564 and 68, 602 and 62 entries at K)."""
    import seld_eval
    name, logits, want = planted
    table = seld_eval.meta_frame_table(SEGMENTS)
    q_n = len(table)
    probs = torch.full((q_n, 648, 13), float("nan"), dtype=torch.float32, device=logits.device)
    cells, scores, counts = seld_eval.grid_decode(logits, 0, table, 0, q_n, THRESHOLD, k, probs=probs)
    got = probs.cpu().double().numpy()
    err = float(np.abs(got - want).max())
    print(f"{name} K={k}: max |P_q - float64| = {err:.3e}")
    assert err <= 2e-5
    ref_dets, near = ref.decode_detections(want, THRESHOLD, k)
    cells, scores, counts = cells.cpu().numpy(), scores.cpu().numpy(), counts.cpu().numpy()
    share = float(near.mean())
    print(f"{name} K={k}: near-tie exclusions {int(near.sum())} of {near.size} ({100 * share:.3f} %), "
          f"{sum(len(c) for r in ref_dets for c in r)} reference detections")
    assert share <= 0.01
    mismatches = []
    for q in range(q_n):
        for c in range(13):
            n = int(counts[q, c])
            assert (cells[q, c, n:] == -1).all() and (scores[q, c, n:] == 0).all()
            assert np.array_equal(scores[q, c, :n], got[q, cells[q, c, :n], c].astype(np.float32))
            if not near[q, c] and cells[q, c, :n].tolist() != ref_dets[q][c]:
                mismatches.append((q, c, cells[q, c, :n].tolist(), ref_dets[q][c]))
    assert not mismatches, mismatches[:5]


def test_streaming_and_splits_are_bit_identical(planted):
    """Launches of 7 windows through the streaming driver, and arbitrary meta-frame ranges over all windows, give the
    outputs of one launch over everything; two runs are bit-identical."""
    import seld_eval
    _, logits, _ = planted
    table = seld_eval.meta_frame_table(SEGMENTS)
    q_n = len(table)

    def whole():
        probs = torch.empty((q_n, 648, 13), dtype=torch.float32, device=logits.device)
        return (*seld_eval.grid_decode(logits, 0, table, 0, q_n, THRESHOLD, 4, probs=probs), probs)

    one = whole()
    again = whole()
    streamed = seld_eval.decode((logits[lo:lo + 7] for lo in range(0, logits.shape[0], 7)), table, THRESHOLD, 4,
                                keep_probs=True)
    split = [torch.empty_like(t) for t in one]
    for lo, hi in ((0, 37), (37, 38), (38, 200), (200, q_n)):
        seld_eval.grid_decode(logits, 0, table, lo, hi - lo, THRESHOLD, 4, out=tuple(t[lo:hi] for t in split[:3]),
                              probs=split[3][lo:hi])
    for a, b, c, d in zip(one, again, streamed, split):
        assert torch.equal(a, b) and torch.equal(a, c) and torch.equal(a, d)


def test_error_paths(gpu_device):
    import seld_eval
    from seld_native import SeldNativeError
    table = seld_eval.meta_frame_table(np.array([[0, 600]]))
    logits = torch.zeros((6, 250, 648, 14), dtype=torch.float32, device=gpu_device)      # windows 2..7 of 12
    out = (torch.full((10, 13, 4), 77, dtype=torch.int32, device=gpu_device),
           torch.full((10, 13, 4), 77.0, dtype=torch.float32, device=gpu_device),
           torch.full((10, 13), 77, dtype=torch.int32, device=gpu_device))
    probs = torch.full((10, 648, 13), 77.0, dtype=torch.float32, device=gpu_device)
    with pytest.raises(SeldNativeError):                                  # meta-frames 0..9 need window 0
        seld_eval.grid_decode(logits, 2, table, 0, 10, 0.5, 4, out=out, probs=probs)
    with pytest.raises(SeldNativeError):                                  # meta-frames 100..109 need windows 9..10
        seld_eval.grid_decode(logits, 2, table, 100, 10, 0.5, 4, out=out, probs=probs)
    torch.cuda.synchronize()
    assert all((t == 77).all() for t in out) and (probs == 77).all()
    ok = seld_eval.grid_decode(logits, 2, table, 60, 10, 0.5, 4)        # frames 300..349 need windows 2..6
    assert (ok[2] == 0).all()
    for k in (0, 9):
        bad = (torch.zeros((10, 13, max(k, 1)), dtype=torch.int32, device=gpu_device),
               torch.zeros((10, 13, max(k, 1)), dtype=torch.float32, device=gpu_device),
               torch.zeros((10, 13), dtype=torch.int32, device=gpu_device))
        with pytest.raises(SeldNativeError):
            seld_eval.grid_decode(logits, 2, table, 60, 10, 0.5, k, out=bad)
    rows = np.array([[3, 2, s, 10 * s - 170, 0] for s in range(9)])    # nine references of class 2 in meta-frame 3
    with pytest.raises(ValueError):
        seld_eval.match_and_score(ok[0], ok[2], seld_eval.meta_frame_table(np.array([[0, 50]])), [rows], 20.0)


def test_match_kernel_matches_brute_force(gpu_device):
    """Random detections and references (0..8 each per entry), with references planted exactly at a cell centre and
    exactly 20 degrees from one along its meridian: stats exact, cost within 1e-9 relative."""
    import seld_eval
    rng = np.random.default_rng(21)
    q_n, k = 60, 8
    det_cell = np.full((q_n, 13, k), -1, np.int32)
    det_count = np.zeros((q_n, 13), np.int32)
    offsets, dirs = [0], []
    exact20 = 0
    for q in range(q_n):
        for c in range(13):
            p = int(rng.integers(0, k + 1))
            det_cell[q, c, :p] = rng.choice(648, size=p, replace=False)
            det_count[q, c] = p
            r = int(rng.integers(0, 9))
            for _ in range(r):
                u = rng.uniform()
                if p and u < 0.4:
                    caz, cel = ref.cell_centre(det_cell[q, c, int(rng.integers(0, p))])
                    el = cel + (20 if rng.uniform() < 0.5 else -20) if u < 0.3 else cel
                    if -90 <= el <= 90:
                        exact20 += u < 0.3
                        dirs.append((int(caz), int(el)))
                        continue
                dirs.append((int(rng.integers(-180, 181)), int(rng.integers(-90, 91))))
            offsets.append(len(dirs))
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(gpu_device)
    stats, cost = seld_eval.doa_match(dev(det_cell), dev(det_count), dev(np.array(offsets, np.int32)),
                                      dev(np.array(dirs, np.int32).reshape(-1, 2)), 20.0)
    stats, cost = stats.cpu().numpy(), cost.cpu().numpy()
    hits20 = 0
    for q in range(q_n):
        for c in range(13):
            lo, hi = offsets[q * 13 + c], offsets[q * 13 + c + 1]
            r, p, kk, tp, cst = ref.match(np.array(dirs[lo:hi]).reshape(-1, 2), det_cell[q, c, :det_count[q, c]])
            assert stats[q, c].tolist() == [r, p, kk, tp], (q, c)
            assert abs(cost[q, c] - cst) <= 1e-9 * abs(cst), (q, c, cost[q, c], cst)
            hits20 += tp
    assert exact20 > 50 and hits20 > 0


def _rows_for_clip(rng, n_frames):
    """Synthetic CSV rows: 0-3 events per meta-frame at distinct cells, same-class sources >= 2 cells apart (azimuth
    wraps), integer DOAs inside their cell, no duplicates; plus rows with 5 m >= n that the evaluation must drop."""
    n_meta = (n_frames + 4) // 5
    rows = []
    for m in range(n_meta):
        placed = []
        for src in range(int(rng.integers(0, 4))):
            for _ in range(100):
                c, i, j = int(rng.integers(0, 13)), int(rng.integers(0, 18)), int(rng.integers(0, 36))
                ok = True
                for c2, i2, j2 in placed:
                    dj = min(abs(j - j2), 36 - abs(j - j2))
                    if (i, j) == (i2, j2) or (c == c2 and max(abs(i - i2), dj) < 2):
                        ok = False
                if ok:
                    placed.append((c, i, j))
                    rows.append([m, c, src, -180 + 10 * j + int(rng.integers(0, 10)), -90 + 10 * i + int(rng.integers(0, 10))])
                    break
    for extra in range(3):
        rows.append([n_meta + 2 * extra, int(rng.integers(0, 13)), 0, 0, 0])
    return np.array(rows, dtype=np.int64).reshape(-1, 5)


def _two_clip_dataset(gpu_device, seed):
    import dataset
    from oracle import features as ofeat
    lengths = (24000 * 7 + 1234, 24000 * 4 + 517)
    clips = [ofeat.synth_pcm(i + seed, 4, n, "noise") for i, n in enumerate(lengths)]
    rng = np.random.default_rng(seed)
    frames = [min(1 + n // 480, dataset.label_frame_count(n / 24000)) for n in lengths]
    rows = [_rows_for_clip(rng, f) for f in frames]
    ds = dataset.SELDDataset.from_pcm(clips, rows, device=gpu_device, use_gaussian_augmentation=False)
    return ds, rows, frames


def test_end_to_end_perfect_predictor(gpu_device, tmp_path):
    """Logits = 20 x the one-hot of the dataset's own labels, in window order: F20 = 1, ER20 = 0, LR_CD = 1 and
    LE_CD <= 7.1 degrees (the largest integer-DOA-to-cell-centre distance, test_seld_eval_cpu); the written CSVs
    rasterise to the labels of the input rows."""
    import dataset
    import seld_eval
    import seld_native
    ds, rows, frames = _two_clip_dataset(gpu_device, 5)
    assert ds.segments.tolist() == [[0, frames[0]], [frames[0], frames[1]]]
    assert all(np.array_equal(a, b) for a, b in zip(ds.metadata_rows, rows))

    def batches():
        for lo in range(0, len(ds), 3):
            _, mask = ds.device_batch(list(range(lo, min(lo + 3, len(ds)))))
            yield 20.0 * seld_native.expand_labels(mask)

    res = seld_eval.evaluate_logits(batches(), ds, events_dir=tmp_path, names=["first", "second"])
    print({k: res[k] for k in ("F20", "ER20", "LE_CD", "LR_CD", "TP", "FP", "FN", "N")})
    assert res["N"] > 100
    assert res["F20"] == 1.0 and res["ER20"] == 0.0 and res["LR_CD"] == 1.0 and res["LE_CD"] <= 7.1
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
    path = tmp_path_factory.mktemp("seld_eval") / "crnn.pth"
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
    """MIOpen's default convolution solutions for the CRNN's shapes are not bitwise repeatable from call to call (the
    same model on the same batch differs by up to one bf16 ulp of the logits); its deterministic mode is."""
    saved = torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark
    torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = True, False
    yield
    torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = saved


def test_evaluate_seld_equals_evaluate_logits_of_the_loaded_model(gpu_device, crnn_checkpoint, tmp_path,
                                                                  deterministic_convolutions):
    """Plumbing: checkpoint loading, window order and batch boundaries.  evaluate_seld on the checkpoint and
    evaluate_logits on the logits of the same model run here over the same batches must agree exactly (the
    untrained model's probabilities sit near 1/14, so one differing logit bit moves detections: the convolutions run in
    MIOpen's deterministic mode, see the fixture)."""
    from torch.utils.data import DataLoader
    import seld_eval
    import trainer
    from utils import safe_torch_load
    ds, _, _ = _two_clip_dataset(gpu_device, 9)
    threshold = 1.0 / 14.0 + 1e-4
    got = trainer.evaluate_seld(DataLoader(ds, batch_size=3, shuffle=False), model_path=crnn_checkpoint,
                                device=gpu_device, threshold=threshold, max_peaks=8, events_dir=tmp_path / "events")
    model = trainer.prepare_model_for_device(trainer.build_model((ds.I, ds.J), True, n_channels=ds.n_channels),
                                             gpu_device)
    model.load_state_dict(safe_torch_load(crnn_checkpoint, map_location=gpu_device)["model_state_dict"])
    model.eval()
    logits = []
    for lo in range(0, len(ds), 3):
        spec, _ = ds.device_batch(list(range(lo, min(lo + 3, len(ds)))))
        with torch.no_grad(), trainer.autocast_context(gpu_device):
            logits.append(model(spec))
    want = seld_eval.evaluate_logits(iter(logits), ds, threshold=threshold, max_peaks=8)
    print({k: got[k] for k in ("F20", "ER20", "LE_CD", "LR_CD", "TP", "FP", "FN", "N")})
    assert got["TP"] + got["FP"] > 0
    for key in ("F20", "ER20", "LE_CD", "LR_CD", "TP", "FP", "FN", "N", "S", "D", "I", "per_class"):
        assert _same(got[key], want[key]), key
    assert len(got["event_files"]) == 2 and got["checkpoint_epoch"] == 0


def test_infer_cli_writes_event_csv(gpu_device, crnn_checkpoint, tmp_path):
    import dataset
    rng = np.random.default_rng(4)
    pcm = (rng.standard_normal((24000 * 10, 4)) * 3000).clip(-32768, 32767).astype("<i2")
    wav = tmp_path / "synthetic_take.wav"
    with wave.open(str(wav), "wb") as wf:
        wf.setnchannels(4)
        wf.setsampwidth(2)
        wf.setframerate(24000)
        wf.writeframes(pcm.tobytes())
    out = tmp_path / "events"
    run = subprocess.run([sys.executable, str(PKG / "infer.py"), "--checkpoint", str(crnn_checkpoint), "--out-dir", str(out),
                          "--model-type", "crnn", "--threshold", str(1.0 / 14.0 + 1e-4), "--max-peaks", "8", str(wav)],
                         capture_output=True, text=True, timeout=600, cwd=str(ROOT))
    print(run.stdout[-2000:], run.stderr[-4000:])
    assert run.returncode == 0
    rows = dataset._read_metadata_rows(out / "synthetic_take.csv")
    assert rows.shape[1] == 5 and rows.shape[0] > 0
    assert ((rows[:, 1] >= 0) & (rows[:, 1] < 13)).all() and ((rows[:, 2] >= 0) & (rows[:, 2] < 8)).all()
    assert rows[:, 0].max() < 100                                  # 10 s = 500 frames = 100 meta-frames
