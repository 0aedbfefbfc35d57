"""GPU checks of the threshold sweep (csrc/seld_sweep.hip, seld_eval.sweep / apply_thresholds / evaluate_logits, infer.py
--thresholds).  Everything is compared against the kernels that were there before
(seld_doa_match, seld_doa_match_dirs, the decode at the threshold itself), never against the code under test; the plain
numpy restatement (tests/seld_sweep_ref.py) is a second witness for the prefix tables."""
import math
import wave
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import seld_eval_ref as ref
import seld_sweep_ref as sref

pytestmark = pytest.mark.gpu

NQ = 37                    # 481 entries: the last 16-lane workgroup of the prefix kernel is partly empty
GRID = sref.GRID


def _bits(t):
    return t.contiguous().view(torch.int64)


# ---------------------------------------------------------------------------------------------- random entries

def _random_entries(k, seed):
    """(det_cell [NQ, 13, K], det_score, det_count, det_dir [NQ, 13, K, 2], offsets [NQ * 13 + 1], dirs [R, 2], refs: list
    per entry, planted: {name: (q, c)}) as numpy.  0..8 references and 0..K detections per entry at random (scores sorted,
    on a 1/64 raster so that many equal a threshold), and the planted entries of the issue."""
    rng = np.random.default_rng(seed)
    cell = np.full((NQ, 13, k), -1, np.int32)
    score = np.zeros((NQ, 13, k), np.float32)
    count = np.zeros((NQ, 13), np.int32)
    refs = []
    for q in range(NQ):
        for c in range(13):
            p = int(rng.integers(0, k + 1))
            cell[q, c, :p] = rng.choice(648, size=p, replace=False)
            score[q, c, :p] = np.sort(rng.integers(2, 65, size=p))[::-1] / 64.0
            count[q, c] = p
            rows = []
            for _ in range(int(rng.integers(0, 9))):
                if p and rng.uniform() < 0.5:                           # near a detection: within 20 degrees more often than not
                    caz, cel = ref.cell_centre(cell[q, c, int(rng.integers(0, p))])
                    rows.append((int(np.clip(caz + rng.integers(-14, 15), -180, 180)),
                                 int(np.clip(cel + rng.integers(-14, 15), -90, 90))))
                else:
                    rows.append((int(rng.integers(-180, 181)), int(rng.integers(-90, 91))))
            refs.append(rows)

    def plant(q, c, cells, rows):
        n = min(len(cells), k)
        cell[q, c], score[q, c], count[q, c] = -1, 0.0, n
        cell[q, c, :n] = cells[:n]
        score[q, c, :n] = np.linspace(0.9, 0.3, n).astype(np.float32)
        refs[q * 13 + c] = list(rows)

    centre = lambda x: tuple(int(v) for v in ref.cell_centre(x))
    some = [100, 137, 211, 290, 333, 402, 475, 590]
    planted = {"no_refs": (0, 0), "no_dets": (0, 1), "empty": (0, 2), "full": (1, 0), "more_refs": (1, 1), "more_dets": (1, 2),
               "duplicates": (2, 0), "meridian20": (2, 1), "hungarian": (2, 2)}
    plant(0, 0, some, [])
    plant(0, 1, [], [centre(x) for x in some[:3]])
    plant(0, 2, [], [])
    plant(1, 0, some, [(centre(x)[0] + 3, centre(x)[1] - 2) for x in reversed(some)])          # R = 8, P = min(8, K)
    plant(1, 1, some[:max(k // 2, 1)], [centre(x) for x in some[:max(k // 2, 1) + 3]])          # R > P
    plant(1, 2, some, [(centre(x)[0] + 1, centre(x)[1]) for x in some[:max(k // 2, 0)]])        # P > R (P = R = 0 at K = 1)
    plant(2, 0, [some[0], some[0], some[1], some[1]], [centre(some[0]), centre(some[1]), centre(some[0])])
    x20 = 9 * 36 + 18                                                                          # centre (5, 5)
    plant(2, 1, [x20, some[3]], [(5, 25), (5, -15)])                                           # exactly 20 degrees, twice
    # the cheapest assignment (A-X, B-Y) has one pair within 20 degrees, the maximum matching two
    plant(2, 2, [9 * 36 + 18, 9 * 36 + 20], [(5, 5), (0, 20)])                                 # X (5, 5), Y (25, 5); A, B
    dirs_of = ref.cell_centre(np.maximum(cell, 0))
    det_dir = np.stack(dirs_of, -1).astype(np.float32) + rng.uniform(-4.0, 4.0, size=(NQ, 13, k, 2)).astype(np.float32)
    det_dir[..., 1] = np.clip(det_dir[..., 1], -90.0, 90.0)
    det_dir[np.arange(k) >= count[..., None]] = 0.0
    offsets = np.concatenate([[0], np.cumsum([len(r) for r in refs])]).astype(np.int32)
    dirs = np.array([d for r in refs for d in r], np.int32).reshape(-1, 2)
    return cell, score, count, det_dir, offsets, dirs, refs, planted


@pytest.fixture(scope="module", params=[1, 4, 8])
def entries(request, gpu_device):
    k = request.param
    host = _random_entries(k, 40 + k)
    dev = tuple(torch.from_numpy(np.ascontiguousarray(a)).to(gpu_device) for a in host[:6])
    return k, host, dev


def test_planted_hungarian_example_is_what_it_claims():
    """The restatement on the planted example: tp = 2, the cost is the assignment with one pair beyond 20 degrees."""
    d = lambda a, b: float(ref.angle_deg(a[0], a[1], b[0], b[1]))
    a, b, x, y = (5, 5), (0, 20), (5, 5), (25, 5)
    assert d(a, x) == 0.0 and d(a, y) <= 20.0 and d(b, x) <= 20.0 and d(b, y) > 20.0
    assert d(a, x) + d(b, y) < d(a, y) + d(b, x)
    r, p, k, tp, cost = ref.match([a, b], [9 * 36 + 18, 9 * 36 + 20])
    assert (r, p, k, tp) == (2, 2, 2, 2) and cost == pytest.approx(d(b, y), abs=1e-12)


def test_prefix_kernel_equals_the_matcher_on_every_prefix(entries):
    """ptp[..., p] / pcost[..., p] against seld_doa_match with the counts clamped to p: tp equal, cost bit-equal; and
    against the numpy restatement: tp exact, cost within 1e-9 relative."""
    import seld_eval
    k, host, (cell, score, count, det_dir, offsets, dirs) = entries
    ptp, pcost = seld_eval.doa_match_prefix(cell, count, offsets, dirs, 20.0)
    assert tuple(ptp.shape) == tuple(pcost.shape) == (NQ, 13, k + 1) and ptp.dtype == torch.int32
    for p in range(k + 1):
        stats, cost = seld_eval.doa_match(cell, count.clamp(max=p), offsets, dirs, 20.0)
        assert torch.equal(ptp[..., p], stats[..., 3]), p
        assert torch.equal(_bits(pcost[..., p]), _bits(cost)), p
    want_tp, want_cost = sref.prefix_tables(host[6], host[0], host[2], k)
    got_tp, got_cost = ptp.cpu().numpy(), pcost.cpu().numpy()
    assert np.array_equal(got_tp, want_tp)
    assert (np.abs(got_cost - want_cost) <= 1e-9 * np.abs(want_cost)).all()
    planted = host[7]
    q, c = planted["hungarian"]
    if k >= 2:
        assert got_tp[q, c, 2] == 2 and got_cost[q, c, 2] > 20.0
    q, c = planted["meridian20"]
    assert got_tp[q, c, 1] == 1 and abs(got_cost[q, c, 1] - 20.0) < 1e-9
    q, c = planted["full"]
    assert host[2][q, c] == k and len(host[6][q * 13 + c]) == 8
    assert int((got_tp[..., k] > 0).sum()) > 50


def test_prefix_kernel_on_directions_equals_the_direction_matcher(entries):
    import seld_eval
    k, host, (cell, score, count, det_dir, offsets, dirs) = entries
    ptp, pcost = seld_eval.doa_match_prefix(None, count, offsets, dirs, 20.0, det_dir=det_dir)
    for p in range(k + 1):
        stats, cost = seld_eval.doa_match_dirs(det_dir, count.clamp(max=p), offsets, dirs, 20.0)
        assert torch.equal(ptp[..., p], stats[..., 3]), p
        assert torch.equal(_bits(pcost[..., p]), _bits(cost)), p
    centres = seld_eval.cell_centre_dirs(cell.clamp(min=0))
    on_centres = seld_eval.doa_match_prefix(None, count, offsets, dirs, 20.0, det_dir=centres)
    on_cells = seld_eval.doa_match_prefix(cell, count, offsets, dirs, 20.0)
    assert torch.equal(on_centres[0], on_cells[0]) and torch.equal(_bits(on_centres[1]), _bits(on_cells[1]))


def test_prefix_kernel_refuses_what_the_matcher_refuses(entries, gpu_device):
    """Nine references, a count above K and a negative count: -1 / NaN at every prefix, the neighbours untouched."""
    import seld_eval
    k, host, (cell, score, count, det_dir, offsets, dirs) = entries
    refs = [list(r) for r in host[6]]
    refs[5 * 13 + 3] = [(10 * i - 40, 0) for i in range(9)]
    offs = torch.from_numpy(np.concatenate([[0], np.cumsum([len(r) for r in refs])]).astype(np.int32)).to(gpu_device)
    drs = torch.from_numpy(np.array([d for r in refs for d in r], np.int32).reshape(-1, 2)).to(gpu_device)
    bad_count = count.clone()
    bad_count[6, 4], bad_count[7, 5] = k + 1, -1
    ptp, pcost = seld_eval.doa_match_prefix(cell, bad_count, offs, drs, 20.0)
    good_tp, good_cost = seld_eval.doa_match_prefix(cell, count, offsets, dirs, 20.0)
    refused = torch.zeros((NQ, 13), dtype=torch.bool, device=gpu_device)
    for q, c in ((5, 3), (6, 4), (7, 5)):
        refused[q, c] = True
        assert (ptp[q, c] == -1).all() and torch.isnan(pcost[q, c]).all()
    assert torch.equal(ptp[~refused], good_tp[~refused]) and torch.equal(_bits(pcost[~refused]), _bits(good_cost[~refused]))
    stats, cost = seld_eval.doa_match(cell, bad_count, offs, drs, 20.0)                       # the matcher's own refusals
    assert (stats[refused][:, 3] == -1).all() and torch.isnan(cost[refused]).all()


def test_prefix_kernel_error_returns(entries, gpu_device):
    import seld_eval
    from seld_native import SeldNativeError
    k, host, (cell, score, count, det_dir, offsets, dirs) = entries
    with pytest.raises(SeldNativeError):
        seld_eval.doa_match_prefix(torch.zeros((NQ, 13, 9), dtype=torch.int32, device=gpu_device), count, offsets, dirs, 20.0)
    with pytest.raises(SeldNativeError):
        seld_eval.doa_match_prefix(cell, count, offsets, dirs, 20.0, I=0)
    with pytest.raises(SeldNativeError):
        seld_eval.doa_match_prefix(cell.cpu(), count.cpu(), offsets.cpu(), dirs.cpu(), 20.0)
    with pytest.raises(ValueError):
        seld_eval.doa_match_prefix(cell, count, offsets[:-1], dirs, 20.0)


# ---------------------------------------------------------------------------------------------- the score kernel

def _rows_by_the_old_path(cell, score, count, offsets, dirs, thresholds):
    import seld_eval
    rows = []
    for t in thresholds:
        cut = seld_eval.apply_thresholds(cell, score, count, [t] * 13)
        rows.append(seld_eval.score(*seld_eval.doa_match(cut[0], cut[2], offsets, dirs, 20.0)))
    return rows


def _assert_rows_equal(swept, rows, where=""):
    """Row t of a sweep against the record of the single-threshold path: counts exact, the costs within 1e-12 relative
    (they are summed in another shape)."""
    def close(a, b):
        return (math.isnan(a) and math.isnan(b)) or abs(a - b) <= 1e-12 * abs(b)

    for t, want in enumerate(rows):
        for key in ("TP", "FP", "FN", "N", "S", "D", "I", "matched", "F20", "ER20", "LR_CD"):
            a, b = swept[key][t], want[key]
            assert a == b or (isinstance(b, float) and math.isnan(a) and math.isnan(b)), (where, t, key, a, b)
        assert close(swept["LE_CD"][t], want["LE_CD"]), (where, t, swept["LE_CD"][t], want["LE_CD"])
        for key in ("TP", "FP", "FN", "N", "F20", "LR_CD"):
            a, b = swept["per_class"][key][t], want["per_class"][key]
            assert all(x == y or (math.isnan(x) and math.isnan(y)) for x, y in zip(a, b)), (where, t, key)
        assert all(close(x, y) for x, y in zip(swept["per_class"]["LE_CD"][t], want["per_class"]["LE_CD"])), (where, t)


@pytest.mark.parametrize("n_thresholds", [1, 7, 64])
def test_score_kernel_equals_score_on_truncated_detections(entries, n_thresholds):
    """T = 1, 7 and 64 thresholds on the 1/64 raster of the scores (so scores equal to a threshold occur at every one),
    chunks of 5 meta-frames (37 = 7 x 5 + 2): counts, S / D / I and per-class counts exactly those of seld_eval.score on
    seld_doa_match of the truncated detections, costs within 1e-12; two runs bit-identical."""
    import seld_eval
    k, host, (cell, score, count, det_dir, offsets, dirs) = entries
    thresholds = {1: [0.5], 7: [4 / 64, 9 / 64, 0.25, 0.5, 0.75, 63 / 64, 1.0], 64: [(i + 1) / 64 for i in range(64)]}[n_thresholds]
    assert int((score == 0.5).sum()) > 0
    swept = seld_eval.sweep(cell, score, count, None, None, thresholds, 20.0, refs=(offsets, dirs), chunk=5)
    assert swept["thresholds"] == thresholds
    rows = _rows_by_the_old_path(cell, score, count, offsets, dirs, thresholds)
    _assert_rows_equal(swept, rows, f"K={k}")
    if n_thresholds > 1:
        assert len({r["TP"] + r["FP"] for r in rows}) >= 3
    for t, row in enumerate(rows):
        tp, fp, fn = row["TP"], row["FP"], row["FN"]
        assert swept["precision"][t] == (tp / (tp + fp) if tp + fp else pytest.approx(math.nan, nan_ok=True))
        assert swept["recall"][t] == (tp / (tp + fn) if tp + fn else pytest.approx(math.nan, nan_ok=True))
    ptp, pcost = seld_eval.doa_match_prefix(cell, count, offsets, dirs, 20.0)
    one = seld_eval.sweep_score(ptp, pcost, score, count, offsets, thresholds, chunk=5)
    two = seld_eval.sweep_score(ptp, pcost, score, count, offsets, thresholds, chunk=5)
    assert tuple(one[0].shape) == (n_thresholds, 8, 13, 5) and tuple(one[1].shape) == (n_thresholds, 8, 3)
    assert tuple(one[2].shape) == (n_thresholds, 8, 13) and one[0].dtype == one[1].dtype == torch.int64
    assert torch.equal(one[0], two[0]) and torch.equal(one[1], two[1]) and torch.equal(_bits(one[2]), _bits(two[2]))
    whole = seld_eval.sweep_score(ptp, pcost, score, count, offsets, thresholds, chunk=1000)     # one chunk: the same sums
    assert torch.equal(one[0].sum(1), whole[0].sum(1)) and torch.equal(one[1].sum(1), whole[1].sum(1))


def test_score_kernel_error_returns(entries):
    import seld_eval
    from seld_native import SeldNativeError
    k, host, (cell, score, count, det_dir, offsets, dirs) = entries
    ptp, pcost = seld_eval.doa_match_prefix(cell, count, offsets, dirs, 20.0)
    for bad in ([], [(i + 1) / 65 for i in range(65)], [0.5, 0.4], [0.5, 0.5], [0.0, 0.5], [-0.1], [0.5, 1.5], [float("nan")]):
        with pytest.raises(SeldNativeError):
            seld_eval.sweep_score(ptp, pcost, score, count, offsets, bad)
    with pytest.raises(ValueError):
        seld_eval.sweep_score(ptp, pcost, score, count, offsets, [0.5], chunk=0)
    with pytest.raises(ValueError):
        seld_eval.sweep_score(ptp[..., :-1], pcost, score, count, offsets, [0.5])
    with pytest.raises(SeldNativeError):
        seld_eval.sweep_score(ptp.cpu(), pcost.cpu(), score.cpu(), count.cpu(), offsets.cpu(), [0.5])


# ---------------------------------------------------------------------------------------------- end to end

@pytest.fixture(scope="module")
def timeline(gpu_device):
    """(fp32 logits [7, 250, 648, 14] on the device, reference rows per segment).  The references come from the decode
    that was there before, at 0.5: most detections get a reference a few degrees off, some none, plus stray rows."""
    import seld_eval
    logits = torch.from_numpy(ref.planted_logits(sref.SEGMENTS, sref.SEED)).to(gpu_device)
    table = seld_eval.meta_frame_table(sref.SEGMENTS)
    cells, _, counts = seld_eval.grid_decode(logits, 0, table, 0, len(table), 0.5, 8)
    cells, counts = cells.cpu().numpy(), counts.cpu().numpy()
    rng = np.random.default_rng(8)
    rows = [[], []]
    for q in range(len(table)):
        s, m = int(table.segment[q]), int(table.index[q])
        for c in range(13):
            for r in range(int(counts[q, c])):
                if rng.uniform() < 0.85:
                    az, el = ref.cell_centre(cells[q, c, r])
                    rows[s].append([m, c, r, int(np.clip(az + rng.integers(-4, 5), -180, 180)),
                                    int(np.clip(el + rng.integers(-4, 5), -90, 90))])
        if rng.uniform() < 0.3:
            rows[s].append([m, int(rng.integers(0, 13)), 7, int(rng.integers(-180, 181)), int(rng.integers(-90, 91))])
    return logits, [np.array(r, dtype=np.int64).reshape(-1, 5) for r in rows]


def _dataset(rows, device):
    return SimpleNamespace(segments=sref.SEGMENTS, metadata_rows=rows, total_frames=sref.TOTAL, I=18, J=36, device=device)


def _batches(logits, patterns=()):
    """Batches of 3 windows; with patterns [P, B, ...]: stack n is the timeline as the model would give it under pattern n."""
    import seld_augment
    if patterns:
        source = lambda p: torch.from_numpy(np.asarray(seld_augment.cell_source(p), dtype=np.int64)).to(logits.device)
        stacks = torch.stack([logits[:, :, source(p), :] for p in patterns])
        return (stacks[:, lo:lo + 3] for lo in range(0, logits.shape[0], 3))
    return (logits[lo:lo + 3] for lo in range(0, logits.shape[0], 3))


METRIC_KEYS = ("F20", "ER20", "LE_CD", "LR_CD", "TP", "FP", "FN", "N", "S", "D", "I", "matched", "per_class")


def _same(a, b):
    if isinstance(a, float) and isinstance(b, float) and math.isnan(a) and math.isnan(b):
        return True
    if isinstance(a, list):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(_same(a[k], b[k]) for k in a)
    return a == b


# (the planted events last one meta-frame, so the default min_len = 3 of track=True leaves only chance tracks: the rows still
#  have to agree; "track-short" keeps every track and scores hundreds of detections)
MODES = {"plain": {}, "tta": {"patterns": (0, 9)}, "refine": {"refine": True}, "track": {"track": True},
         "track-refine": {"track": True, "refine": True}, "track-short": {"track": {"min_len": 1, "max_gap": 1}}}


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("mode", list(MODES))
def test_sweep_rows_equal_single_threshold_evaluations(timeline, gpu_device, dtype, mode):
    """Row t of evaluate_logits(sweep=grid) is evaluate_logits(threshold=t), for the seven thresholds of the grid (0.05 and
    0.08 decode far more than 0.5 does, 0.97 less); the main result is the one without the sweep."""
    import seld_eval
    logits, rows = timeline
    logits = logits.to(torch.bfloat16) if dtype == "bf16" else logits
    ds = _dataset(rows, gpu_device)
    kw = MODES[mode]
    batches = lambda: _batches(logits, kw.get("patterns", ()))
    plain = seld_eval.evaluate_logits(batches(), ds, threshold=0.5, max_peaks=8, **kw)
    swept = seld_eval.evaluate_logits(batches(), ds, threshold=0.5, max_peaks=8, sweep=GRID, **kw)
    assert "sweep" not in plain and "class_thresholds" not in plain and "class_thresholds" not in swept
    assert _same({k: v for k, v in swept.items() if k != "sweep"}, plain)
    sw = swept["sweep"]
    assert sw["thresholds"] == [float(np.float32(t)) for t in GRID]
    singles = [seld_eval.evaluate_logits(batches(), ds, threshold=t, max_peaks=8, **kw) for t in GRID]
    _assert_rows_equal(sw, singles, f"{dtype} {mode}")
    totals = [r["TP"] + r["FP"] for r in singles]
    print(f"{dtype} {mode}: detections {totals}, F20 {[round(r['F20'], 4) for r in singles]}, best {sw['best']}")
    assert len(set(totals)) >= 3 and (plain["TP"] > 50 or kw.get("track") is True)
    f20 = sw["F20"]
    assert sw["best"]["global"] in sw["thresholds"] and f20[sw["thresholds"].index(sw["best"]["global"])] == max(f20)
    assert len(sw["best"]["per_class"]) == 13


def test_class_thresholds_reproduce_a_single_threshold_and_mix_per_class(timeline, gpu_device, tmp_path):
    """class_thresholds = [t] * 13 gives the metrics and the event CSV bytes of threshold = t (decoded at t itself); a
    mixed vector gives each class the TP / FP / FN of the single-threshold run at its own value."""
    import seld_eval
    logits, rows = timeline
    ds = _dataset(rows, gpu_device)
    singles = {}
    for t in (0.08, 0.2, 0.5, 0.9):
        singles[t] = seld_eval.evaluate_logits(_batches(logits), ds, threshold=t, max_peaks=4, events_dir=tmp_path / f"t{t}")
    for t in (0.2, 0.9):
        got = seld_eval.evaluate_logits(_batches(logits), ds, class_thresholds=[t] * 13, max_peaks=4,
                                        events_dir=tmp_path / f"c{t}", sweep=(0.05, 0.5))       # a lower decode threshold
        assert got["class_thresholds"] == [float(np.float32(t))] * 13
        for key in METRIC_KEYS:
            assert _same(got[key], singles[t][key]), (t, key)
        for a, b in zip(got["event_files"], singles[t]["event_files"]):
            assert Path(a).read_bytes() == Path(b).read_bytes() and Path(a).stat().st_size > 0
    mixed = [(0.08, 0.2, 0.5, 0.9)[c % 4] for c in range(13)]
    got = seld_eval.evaluate_logits(_batches(logits), ds, class_thresholds=mixed, max_peaks=4)
    for c, t in enumerate(mixed):
        for key in ("TP", "FP", "FN", "N"):
            assert got["per_class"][key][c] == singles[t]["per_class"][key][c], (c, key)
    assert len({singles[t]["FP"] for t in singles}) >= 3
    with pytest.raises(ValueError):
        seld_eval.evaluate_logits(_batches(logits), ds, threshold=0.5, class_thresholds=mixed)


# ---------------------------------------------------------------------------------------------- thresholds file -> infer.py

@pytest.fixture
def deterministic_convolutions():
    """MIOpen's default convolution solutions are not bitwise repeatable from call to call; its deterministic mode is (the
    untrained model's probabilities sit near 1 / 14, so one differing logit bit moves detections)."""
    saved = torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark
    torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = True, False
    yield
    torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = saved


def test_thresholds_file_drives_infer(gpu_device, tmp_path, deterministic_convolutions):
    """A sweep writes thresholds.json; infer.py --thresholds on the recording writes the CSV of
    evaluate_logits(class_thresholds=that file) on the same model's logits, whatever --threshold says."""
    import dataset
    import infer
    import seld_eval
    import trainer
    saved = trainer.config.MODEL_TYPE
    try:
        trainer.config.MODEL_TYPE = "crnn"
        torch.manual_seed(0)
        model = trainer.prepare_model_for_device(trainer.build_model((18, 36), True, n_channels=4), gpu_device).eval()
        checkpoint = tmp_path / "crnn.pth"
        torch.save({"epoch": 0, "model_state_dict": trainer.model_state_dict(model), "train_loss": 0.0, "test_loss": 0.0},
                   checkpoint)
        rng = np.random.default_rng(4)
        pcm = (rng.standard_normal((24000 * 6, 4)) * 3000).clip(-32768, 32767).astype("<i2")
        wav = tmp_path / "take.wav"
        with wave.open(str(wav), "wb") as wf:
            wf.setnchannels(4)
            wf.setsampwidth(2)
            wf.setframerate(24000)
            wf.writeframes(pcm.tobytes())
        rows = np.array([[m, int(rng.integers(0, 13)), 0, int(rng.integers(-180, 181)), int(rng.integers(-90, 91))]
                         for m in range(0, 60, 2)], dtype=np.int64)
        samples, rate = infer._pcm(wav)
        ds = dataset.SELDDataset.from_pcm([samples], [rows], sample_rate=rate, device=gpu_device,
                                          use_gaussian_augmentation=False)
        logits = lambda: trainer.timeline_logits(model, ds, 4, gpu_device)
        base = 1.0 / 14.0
        file = tmp_path / "thresholds.json"
        swept = seld_eval.evaluate_logits(logits(), ds, threshold=base + 1e-4, max_peaks=8,
                                          sweep=[base + 1e-4, base + 3e-4, base + 1e-3, base + 3e-3], thresholds_out=file)
        assert swept["thresholds_file"] == str(file) and swept["N"] == 30
        doc = seld_eval.load_thresholds(file, max_peaks=8, tta_patterns=(), refine=False)
        assert doc["global"] == swept["sweep"]["best"]["global"] and doc["per_class"] == swept["sweep"]["best"]["per_class"]
        assert doc["grid"]["thresholds"] == swept["sweep"]["thresholds"]
        want = seld_eval.evaluate_logits(logits(), ds, class_thresholds=file, max_peaks=8, events_dir=tmp_path / "want",
                                         names=["take"], sweep=())
        assert want["class_thresholds"] == doc["per_class"]
        written = infer.main(["--checkpoint", str(checkpoint), "--out-dir", str(tmp_path / "got"), "--model-type", "crnn",
                              "--thresholds", str(file), "--threshold", "0.9", "--max-peaks", "8", "--batch-size", "4",
                              "--device", str(gpu_device), str(wav)])
        assert Path(written[0]).read_bytes() == Path(want["event_files"][0]).read_bytes()
        assert Path(written[0]).stat().st_size > 0
    finally:
        trainer.config.MODEL_TYPE = saved
