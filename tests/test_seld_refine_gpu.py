"""GPU checks of the sub-cell DOA refinement (csrc/seld_refine.hip, seld_eval.py, infer.py) against the float64 restatement
of DESIGN.md section 15.1 (tests/seld_refine_ref.py).  Every test goes through seld_grid_decode_refine or
seld_doa_match_dirs."""
import ctypes
from pathlib import Path
from types import SimpleNamespace
import wave

import numpy as np
import pytest
import torch

import seld_eval_ref as ref
import seld_refine_ref as rref
import seld_tta_ref as tref

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
PKG = ROOT / "sound-event-localization-detection_amd"
SEGMENTS = np.array([[0, 503], [503, 250]])       # 16 windows: a tail window, a window across the segments, partial meta-frames
TOTAL = 753
THRESHOLD = 0.5
SEEDS = {"fp32": 1234, "bf16": 1235}
# Nine fp32 multiply-adds in three components (relative 2^-24 each, |v| >= the peak's own P >= threshold of a sum of at
# most nine terms) and two single-precision atan2 (a few ulp of a value below pi): ~1e-5 degrees; the restatement's own
# fp32-against-float64 summation measures 6e-6.  1e-3 leaves two orders of magnitude.
DIR_BOUND_DEG = 1e-3


@pytest.fixture(scope="module", params=["fp32", "bf16"])
def planted(request, gpu_device):
    """(dtype name, device logits [16, 250, 648, 14])."""
    t = torch.from_numpy(ref.planted_logits(SEGMENTS, SEEDS[request.param]))
    if request.param == "bf16":
        t = t.to(torch.bfloat16)
    return request.param, t.to(gpu_device)


def _worst_angle(dirs, probs, cells, counts):
    """Largest great-circle angle between the kernel's directions and the restatement on the kernel's own cells and P_q."""
    probs, cells, counts = probs.cpu().numpy(), cells.cpu().numpy(), counts.cpu().numpy()
    want = rref.refine_detections(probs, cells, counts)
    got = dirs.cpu().numpy().astype(np.float64)
    live = np.arange(cells.shape[-1])[None, None, :] < counts[..., None]
    assert (got[~live] == 0).all()                                      # entries past the count
    assert (got[live][:, 0] >= -180.0).all() and (got[live][:, 0] < 180.0).all()
    return float(rref.angle(got[live], want[live]).max()) if live.any() else 0.0


@pytest.mark.parametrize("k", [1, 8])
def test_refined_decode_matches_the_restatement(planted, k):
    """cells, scores, counts and P_q are grid_decode's bit for bit; every det_dir is within 1e-3 degrees (great-circle) of
    the float64 restatement on the kernel's own cells and fp32 P_q; the case has detections in the pole rows and at the
    azimuth seam."""
    import seld_eval
    name, logits = planted
    table = seld_eval.meta_frame_table(SEGMENTS)
    q_n = len(table)
    probs = torch.full((q_n, 648, 13), float("nan"), dtype=torch.float32, device=logits.device)
    probs_r = torch.full_like(probs, float("nan"))
    plain = seld_eval.grid_decode(logits, 0, table, 0, q_n, THRESHOLD, k, probs=probs)
    cells, scores, counts, dirs = seld_eval.grid_decode_refine(logits, 0, table, 0, q_n, THRESHOLD, k, probs=probs_r)
    assert tuple(dirs.shape) == (q_n, 13, k, 2) and dirs.dtype == torch.float32
    assert torch.equal(cells, plain[0]) and torch.equal(scores, plain[1]) and torch.equal(counts, plain[2])
    assert torch.equal(probs_r, probs)
    live = cells.cpu().numpy()[np.arange(k)[None, None, :] < counts.cpu().numpy()[..., None]]
    rows, cols = set((live // 36).tolist()), set((live % 36).tolist())
    assert {0, 17} <= rows and {0, 35} <= cols, (sorted(rows), sorted(cols))
    worst = _worst_angle(dirs, probs_r, cells, counts)
    centre = seld_eval.cell_centre_dirs(cells).cpu().numpy()[np.arange(k)[None, None, :] < counts.cpu().numpy()[..., None]]
    moved = rref.angle(dirs.cpu().numpy()[np.arange(k)[None, None, :] < counts.cpu().numpy()[..., None]], centre)
    print(f"{name} K={k}: {len(live)} detections, max angle to the restatement {worst:.2e} deg, moved from the centre by "
          f"mean {moved.mean():.3f} max {moved.max():.3f} deg")
    assert len(live) > 200
    assert worst <= DIR_BOUND_DEG
    # inside the hull of the neighbourhood's centres (a diagonal neighbour is 14.1 degrees away), and not the centre
    assert moved.max() <= 14.2 and (moved > 1e-3).mean() > 0.5


def test_tta_walk(planted, gpu_device):
    """patterns = (0,) is the plain walk bit for bit; a three-pattern stack meets the 1e-3 degrees against the restatement
    on the kernel's own P_q, and its other outputs are grid_decode_tta's."""
    import seld_eval
    _, logits = planted
    table = seld_eval.meta_frame_table(SEGMENTS)
    q_n = len(table)
    one = seld_eval.grid_decode_refine(logits, 0, table, 0, q_n, THRESHOLD, 4)
    same = seld_eval.grid_decode_refine(logits[None], 0, table, 0, q_n, THRESHOLD, 4, patterns=(0,))
    assert all(torch.equal(a, b) for a, b in zip(one, same))
    _, patterns, x, _ = tref.case("fp32-three")
    stack = torch.from_numpy(x).to(gpu_device)
    table3 = seld_eval.meta_frame_table(tref.SEG)
    q3 = len(table3)
    probs, probs_r = (torch.full((q3, 648, 13), float("nan"), dtype=torch.float32, device=gpu_device) for _ in range(2))
    plain = seld_eval.grid_decode_tta(stack, patterns, 0, table3, 0, q3, tref.THRESHOLD, 8, probs=probs)
    cells, scores, counts, dirs = seld_eval.grid_decode_refine(stack, 0, table3, 0, q3, tref.THRESHOLD, 8, probs=probs_r,
                                                               patterns=patterns)
    assert torch.equal(cells, plain[0]) and torch.equal(scores, plain[1]) and torch.equal(counts, plain[2])
    assert torch.equal(probs_r, probs)
    worst = _worst_angle(dirs, probs_r, cells, counts)
    print(f"three patterns {patterns}: {int(counts.sum())} detections, max angle to the restatement {worst:.2e} deg")
    assert int(counts.sum()) > 30
    assert worst <= DIR_BOUND_DEG


def test_streaming_and_splits_are_bit_identical(planted):
    """Launches of 7 windows through decode(refine=True), and arbitrary meta-frame ranges over all windows, give one
    launch's det_dir (and the rest) bit for bit; two runs are identical."""
    import seld_eval
    _, logits = planted
    table = seld_eval.meta_frame_table(SEGMENTS)
    q_n = len(table)
    one = seld_eval.grid_decode_refine(logits, 0, table, 0, q_n, THRESHOLD, 4)
    again = seld_eval.grid_decode_refine(logits, 0, table, 0, q_n, THRESHOLD, 4)
    streamed = seld_eval.decode((logits[lo:lo + 7] for lo in range(0, logits.shape[0], 7)), table, THRESHOLD, 4,
                                refine=True)
    assert len(streamed) == 5 and streamed[3] is None
    streamed = (streamed[0], streamed[1], streamed[2], streamed[4])
    split = [torch.full_like(t, 77) for t in one]
    for lo, hi in ((0, 37), (37, 38), (38, 120), (120, q_n)):
        seld_eval.grid_decode_refine(logits, 0, table, lo, hi - lo, THRESHOLD, 4, out=tuple(t[lo:hi] for t in split))
    assert int(one[2].sum()) > 200
    for a, b, c, d in zip(one, again, streamed, split):
        assert torch.equal(a, b) and torch.equal(a, c) and torch.equal(a, d)


def _match_case(rng, q_n=60, k=8):
    """The case of test_seld_eval_gpu.test_match_kernel_matches_brute_force: random detections and references (0..8 each
    per entry), references planted at a cell centre and exactly 20 degrees from one."""
    det_cell = np.full((q_n, 13, k), -1, np.int32)
    det_count = np.zeros((q_n, 13), np.int32)
    offsets, dirs = [0], []
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
                        dirs.append((int(caz), int(el)))
                        continue
                dirs.append((int(rng.integers(-180, 181)), int(rng.integers(-90, 91))))
            offsets.append(len(dirs))
    return det_cell, det_count, np.array(offsets, np.int32), np.array(dirs, np.int32).reshape(-1, 2)


def test_match_dirs_reproduces_doa_match_on_cell_centres(gpu_device):
    """Cell centres as floats: seld_doa_match's stats and cost bit for bit."""
    import seld_eval
    det_cell, det_count, offsets, dirs = _match_case(np.random.default_rng(21))
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(gpu_device)
    stats, cost = seld_eval.doa_match(dev(det_cell), dev(det_count), dev(offsets), dev(dirs), 20.0)
    centres = seld_eval.cell_centre_dirs(dev(det_cell))
    stats_d, cost_d = seld_eval.doa_match_dirs(centres, dev(det_count), dev(offsets), dev(dirs), 20.0)
    assert int(stats[..., 3].sum()) > 0 and int(stats[..., 2].sum()) > 500
    assert torch.equal(stats, stats_d)
    assert torch.equal(cost.view(torch.int64), cost_d.view(torch.int64))


def test_match_dirs_matches_brute_force(gpu_device):
    """Random float directions (fp32 values) against the brute-force restatement: stats exact, cost within 1e-9 relative;
    the seed leaves no pair within 1e-4 degrees of the 20 degree threshold (asserted), so no count hangs on rounding."""
    import seld_eval
    rng = np.random.default_rng(31)
    q_n, k = 40, 8
    det_dir = np.zeros((q_n, 13, k, 2), np.float32)
    det_count = rng.integers(0, k + 1, size=(q_n, 13)).astype(np.int32)
    det_dir[..., 0] = rng.uniform(-180.0, 180.0, size=(q_n, 13, k))
    det_dir[..., 1] = np.degrees(np.arcsin(rng.uniform(-1.0, 1.0, size=(q_n, 13, k))))
    offsets, dirs = [0], []
    for q in range(q_n):
        for c in range(13):
            for _ in range(int(rng.integers(0, 9))):
                p = int(det_count[q, c])
                if p and rng.uniform() < 0.5:                                    # near a detection: most are matches
                    az, el = det_dir[q, c, int(rng.integers(0, p))]
                    dirs.append((int(np.clip(np.rint(az + rng.uniform(-12, 12)), -180, 180)),
                                 int(np.clip(np.rint(el + rng.uniform(-12, 12)), -90, 90))))
                else:
                    dirs.append((int(rng.integers(-180, 181)), int(rng.integers(-90, 91))))
            offsets.append(len(dirs))
    offsets, dirs = np.array(offsets, np.int32), np.array(dirs, np.int32).reshape(-1, 2)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(gpu_device)
    stats, cost = seld_eval.doa_match_dirs(dev(det_dir), dev(det_count), dev(offsets), dev(dirs), 20.0)
    stats, cost = stats.cpu().numpy(), cost.cpu().numpy()
    closest, hits, pairs = np.inf, 0, 0
    for q in range(q_n):
        for c in range(13):
            r = dirs[offsets[q * 13 + c]:offsets[q * 13 + c + 1]].astype(np.float64)
            d = det_dir[q, c, :det_count[q, c]].astype(np.float64)
            dist = ref.angle_deg(r[:, None, 0], r[:, None, 1], d[None, :, 0], d[None, :, 1]) if len(r) and len(d) \
                else np.zeros((len(r), len(d)))
            if dist.size:
                closest = min(closest, float(np.abs(dist - 20.0).min()))
                pairs += dist.size
            kk, tp, cst = ref.match_dist(dist, 20.0)
            assert stats[q, c].tolist() == [len(r), len(d), kk, tp], (q, c)
            assert abs(cost[q, c] - cst) <= 1e-9 * abs(cst), (q, c, cost[q, c], cst)
            hits += tp
    print(f"{pairs} pairs, closest to the threshold {closest:.2e} deg, {hits} matches")
    assert closest > 1e-4
    assert hits > 300


def _bump_logits(probs, device):
    """log P of the synthetic maps as window logits [W, 250, 648, 14] fp32: every frame of meta-frame q carries P[q]; rows
    past the timeline's end are zeros."""
    n_meta = probs.shape[0]
    total = 5 * n_meta
    with np.errstate(divide="ignore"):                                  # a class without a source is P = 0: logit -inf
        logp = torch.from_numpy(np.log(probs)).to(device=device, dtype=torch.float32)
    n_w = (total + 49) // 50
    frame = torch.arange(250, device=device)[None, :] + 50 * torch.arange(n_w, device=device)[:, None]     # [W, 250]
    logits = logp[torch.clamp(frame, max=total - 1) // 5]
    logits[frame >= total] = 0.0
    return logits, total


def _dataset(rows, total, device):
    return SimpleNamespace(segments=np.array([[0, total]]), metadata_rows=[rows], total_frames=total, I=18, J=36,
                           device=device)


def _wrap(az):
    return np.where(az >= 180, az - 360, az)


def test_end_to_end_on_synthetic_bumps(gpu_device, tmp_path):
    """The CPU test's sigma = 6 degree maps as logits, integer-degree reference rows at the true directions:
    evaluate_logits(refine=True) counts what refine=False counts (as the restatement does), its LE_CD is strictly lower
    and at most half, and agrees with the restatement's; the CSV holds directions off the 10-degree raster."""
    import dataset
    import seld_eval
    probs, sources = rref.bump_maps(20)
    logits, total = _bump_logits(probs, gpu_device)
    rows = np.array([[q, c, 0, int(_wrap(np.rint(az))), int(np.rint(el))] for q, c, az, el in sources], dtype=np.int64)
    ds = _dataset(rows, total, gpu_device)
    batches = lambda: (logits[lo:lo + 4] for lo in range(0, logits.shape[0], 4))
    off = seld_eval.evaluate_logits(batches(), ds, threshold=rref.BUMP_THRESHOLD, max_peaks=4, events_dir=tmp_path / "off",
                                    refine=False)
    on = seld_eval.evaluate_logits(batches(), ds, threshold=rref.BUMP_THRESHOLD, max_peaks=4, events_dir=tmp_path / "on",
                                   refine=True)
    assert off["refine"] is False and on["refine"] is True
    # the restatement: its own detections, both directions, against the same integer rows
    dets, _ = ref.decode_detections(probs[..., :13], rref.BUMP_THRESHOLD, 4)
    want = {}
    for mode in ("centre", "refined"):
        stats, cost = np.zeros((100, 13, 4), np.int64), np.zeros((100, 13))
        for q in range(100):
            for c in range(13):
                r = rows[(rows[:, 0] == q) & (rows[:, 1] == c)][:, 3:5].astype(np.float64)
                d = np.array([ref.cell_centre(x) if mode == "centre" else rref.refine(probs[q, :, c], x)
                              for x in dets[q][c]], dtype=np.float64).reshape(-1, 2)
                dist = ref.angle_deg(r[:, None, 0], r[:, None, 1], d[None, :, 0], d[None, :, 1]) if len(r) and len(d) \
                    else np.zeros((len(r), len(d)))
                kk, tp, cst = ref.match_dist(dist, 20.0)
                stats[q, c], cost[q, c] = (len(r), len(d), kk, tp), cst
        want[mode] = ref.metrics(stats, cost)
    print({k: (off[k], on[k]) for k in ("TP", "FP", "FN", "N", "LE_CD")},
          {k: (want["centre"][k], want["refined"][k]) for k in ("TP", "FP", "FN", "N", "LE_CD")})
    for key in ("TP", "FP", "FN", "N"):
        assert off[key] == want["centre"][key] and on[key] == want["refined"][key], key
        if want["centre"][key] == want["refined"][key]:
            assert on[key] == off[key], key
    assert on["N"] == 300 and on["TP"] == 300
    assert on["LE_CD"] < off["LE_CD"] and on["LE_CD"] <= 0.5 * off["LE_CD"]
    assert abs(off["LE_CD"] - want["centre"]["LE_CD"]) <= 1e-9
    assert abs(on["LE_CD"] - want["refined"]["LE_CD"]) <= DIR_BOUND_DEG
    plain = dataset._read_metadata_rows(off["event_files"][0])
    fine = dataset._read_metadata_rows(on["event_files"][0])
    assert plain.shape == fine.shape == (300, 5) and np.array_equal(plain[:, :3], fine[:, :3])
    assert (plain[:, 3] % 10 == 5).all() and (plain[:, 4] % 10 == 5).all()
    assert ((fine[:, 3] % 10 != 5) | (fine[:, 4] % 10 != 5)).mean() > 0.9
    assert (fine[:, 3] >= -180).all() and (fine[:, 3] < 180).all()


def test_end_to_end_with_tracks(gpu_device, tmp_path):
    """Sources that hold still for four meta-frames, one of them blanked for one: with track=True the refined evaluation
    runs, every non-fill row of the CSV carries its detection's refined direction, the fill its cell centre."""
    import dataset
    import seld_eval
    probs, sources = rref.bump_maps(23, hold=4)
    probs = probs.copy()
    q_b, c_b = next((q, c) for q, c, _, _ in sources if q % 4 == 1)
    probs[q_b, :, 13] += probs[q_b, :, c_b]
    probs[q_b, :, c_b] = 0.0
    logits, total = _bump_logits(probs, gpu_device)
    rows = np.array([[q, c, 0, int(_wrap(np.rint(az))), int(np.rint(el))] for q, c, az, el in sources], dtype=np.int64)
    ds = _dataset(rows, total, gpu_device)
    batches = lambda: (logits[lo:lo + 4] for lo in range(0, logits.shape[0], 4))
    res = seld_eval.evaluate_logits(batches(), ds, threshold=rref.BUMP_THRESHOLD, max_peaks=4, events_dir=tmp_path,
                                    track=True, refine=True)
    print({k: res[k] for k in ("TP", "FP", "FN", "N", "LE_CD", "tracking")})
    assert res["refine"] is True and res["tracking"]["filled"] == 1 and res["tracking"]["removed"] == 0
    assert res["TP"] == res["N"] == 300
    table = seld_eval.meta_frame_table(ds.segments, total)
    cells, _, counts, _, dirs = seld_eval.decode(batches(), table, rref.BUMP_THRESHOLD, 4, refine=True)
    cells, counts, dirs = cells.cpu().numpy(), counts.cpu().numpy(), dirs.cpu().numpy()
    events = dataset._read_metadata_rows(res["event_files"][0])
    assert events.shape == (300, 5)
    fills = 0
    for m, c, _, az, el in events.tolist():
        n = int(counts[m, c])
        if n == 0:                                                      # the blanked frame: the track's last cell, its centre
            assert (m, c) == (q_b, c_b) and az % 10 == 5 and el % 10 == 5
            fills += 1
            continue
        assert n == 1
        want_az, want_el = np.rint(dirs[m, c, 0].astype(np.float64))
        assert (az, el) == (int(_wrap(want_az)), int(want_el)), (m, c)
    assert fills == 1
    assert ((events[:, 3] % 10 != 5) | (events[:, 4] % 10 != 5)).mean() > 0.9


def test_error_paths(gpu_device):
    """Null cell_unit / det_dir, K outside 1..8, a duplicate pattern and n_patterns = 17 each return -1 with nothing
    written; so does a host call on CPU tensors (no fallback)."""
    import seld_eval
    import seld_native
    from seld_native import SeldNativeError, _p, _stream_ptr
    seld_native.ensure_init(gpu_device)
    lib = seld_native.load_library()
    table = seld_eval.meta_frame_table(np.array([[0, 100]]))
    first, length = table.device(gpu_device)
    logits = torch.zeros((2, 2, 250, 648, 14), dtype=torch.float32, device=gpu_device)
    unit = seld_eval.cell_unit_table(gpu_device)
    out = (torch.full((20, 13, 8), 77, dtype=torch.int32, device=gpu_device),
           torch.full((20, 13, 8), 77.0, dtype=torch.float32, device=gpu_device),
           torch.full((20, 13), 77, dtype=torch.int32, device=gpu_device),
           torch.full((20, 13, 8, 2), 77.0, dtype=torch.float32, device=gpu_device))
    probs = torch.full((20, 648, 13), 77.0, dtype=torch.float32, device=gpu_device)

    def call(patterns, k, cell_unit, det_dir):
        pats = np.asarray(patterns, dtype=np.int32)
        return lib.seld_grid_decode_refine(_p(logits), 0, 0, 2, 2, 100, _p(first), _p(length), 0, 20,
                                           pats.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)) if len(pats) else None,
                                           len(pats), 0.5, k, cell_unit, _p(out[0]), _p(out[1]), _p(out[2]), det_dir,
                                           _p(probs), _stream_ptr(gpu_device))

    assert call((), 4, None, _p(out[3])) == -1
    assert call((), 4, _p(unit), None) == -1
    assert call((0, 1), 0, _p(unit), _p(out[3])) == -1
    assert call((0, 1), 9, _p(unit), _p(out[3])) == -1
    assert call((3, 3), 4, _p(unit), _p(out[3])) == -1
    assert call(tuple(range(16)) + (0,), 4, _p(unit), _p(out[3])) == -1
    assert lib.seld_doa_match_dirs(None, _p(out[2]), 8, _p(out[2]), _p(out[2]), 20, 20.0, _p(out[0]), _p(probs),
                                   _stream_ptr(gpu_device)) == -1
    torch.cuda.synchronize()
    assert all((t == 77).all() for t in out) and (probs == 77).all()
    for k in (0, 9):
        with pytest.raises(SeldNativeError):
            seld_eval.grid_decode_refine(logits[0], 0, table, 0, 20, 0.5, k)
    with pytest.raises(SeldNativeError):
        seld_eval.grid_decode_refine(logits[:, :1], 0, table, 0, 20, 0.5, 4, patterns=(2, 5))    # window 1 is missing
    with pytest.raises(SeldNativeError):
        seld_eval.grid_decode_refine(logits[0].cpu(), 0, table, 0, 20, 0.5, 4)
    with pytest.raises(ValueError):
        seld_eval.match_and_score(out[0], out[2], table, [np.zeros((0, 5), np.int64)], 20.0, refine=True)
    ok = seld_eval.grid_decode_refine(logits, 0, table, 0, 20, 0.5, 4, patterns=(2, 5))           # uniform maps: nothing
    assert int(ok[2].sum()) == 0 and not ok[3].any()
    assert call((2, 5), 8, _p(unit), _p(out[3])) == 0
    torch.cuda.synchronize()
    assert (out[2] == 0).all() and (out[3] == 0).all() and (out[0] == -1).all()


@pytest.fixture(scope="module")
def crnn_checkpoint(gpu_device, tmp_path_factory):
    """A seeded, untrained CRNN written in the trainer's checkpoint format."""
    import trainer
    old = trainer.config.MODEL_TYPE
    trainer.config.MODEL_TYPE = "crnn"
    torch.manual_seed(0)
    model = trainer.prepare_model_for_device(trainer.build_model((18, 36), True, n_channels=4), gpu_device)
    path = tmp_path_factory.mktemp("seld_refine") / "crnn.pth"
    torch.save({"epoch": 0, "model_state_dict": trainer.model_state_dict(model), "train_loss": 0.0, "test_loss": 0.0},
               path)
    yield path
    trainer.config.MODEL_TYPE = old


@pytest.fixture
def deterministic_convolutions():
    """MIOpen's default convolution solutions for the CRNN's shapes are not bitwise repeatable from call to call; its
    deterministic mode is (the untrained model's probabilities sit near 1/14, so one logit bit moves detections)."""
    saved = torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark
    torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = True, False
    yield
    torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = saved


def test_infer_cli_refine_changes_only_the_directions(gpu_device, crnn_checkpoint, tmp_path, deterministic_convolutions):
    """infer.py's command line with and without --refine on one recording (its main() run here, so that both runs share the
    deterministic convolutions): the rows differ only in the last two columns, and --refine leaves the raster."""
    import dataset
    import infer
    rng = np.random.default_rng(4)
    pcm = (rng.standard_normal((24000 * 6, 4)) * 3000).clip(-32768, 32767).astype("<i2")
    wav = tmp_path / "synthetic_take.wav"
    with wave.open(str(wav), "wb") as wf:
        wf.setnchannels(4)
        wf.setsampwidth(2)
        wf.setframerate(24000)
        wf.writeframes(pcm.tobytes())
    common = ["--checkpoint", str(crnn_checkpoint), "--model-type", "crnn", "--threshold", str(1.0 / 14.0 + 1e-4),
              "--max-peaks", "8", "--device", str(gpu_device)]
    assert infer.parse_args(common + ["--out-dir", "x", str(wav)]).refine is False
    plain = infer.main(common + ["--out-dir", str(tmp_path / "plain"), str(wav)])
    fine = infer.main(common + ["--out-dir", str(tmp_path / "fine"), "--refine", str(wav)])
    a, b = dataset._read_metadata_rows(plain[0]), dataset._read_metadata_rows(fine[0])
    assert a.shape == b.shape and a.shape[0] > 0 and a.shape[1] == 5
    assert np.array_equal(a[:, :3], b[:, :3])
    assert (a[:, 3] % 10 == 5).all() and (a[:, 4] % 10 == 5).all()
    assert not np.array_equal(a[:, 3:], b[:, 3:])
    assert (b[:, 3] >= -180).all() and (b[:, 3] < 180).all() and (np.abs(b[:, 4]) <= 90).all()
    d = ref.angle_deg(a[:, 3], a[:, 4], b[:, 3], b[:, 4])
    assert d.max() <= 15.0             # inside the hull of the neighbours' centres (14.1 degrees) plus the rounding
