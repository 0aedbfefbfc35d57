"""GPU checks of the segment-based, class-macro SELD metrics (csrc/seld_segment.hip, seld_eval.doa_assign / segment_score /
jackknife_score / segment_metrics / evaluate_logits) against the plain float64 restatement
(tests/seld_segment_ref.py) and, for the assignment's total, against seld_doa_match itself."""
import ctypes
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import seld_eval_ref as ref
import seld_segment_ref as sg

pytestmark = pytest.mark.gpu

Q = int(sg.SEG_OFFSETS[-1])                    # 40 meta-frames: 520 entries, the last 16-lane workgroup is half empty
SEGMENTS = np.array([[0, 113], [113, 50], [163, 33]])      # frames: 23, 10 and 7 meta-frames, each recording ends on a partial one


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _close(got, want, rel):
    """nan-aware |got - want| <= rel |want|, elementwise over arrays."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    both_nan = np.isnan(got) & np.isnan(want)
    with np.errstate(invalid="ignore"):
        return bool((both_nan | (np.abs(got - want) <= rel * np.abs(want))).all())


def _table():
    import seld_eval
    table = seld_eval.meta_frame_table(SEGMENTS)
    assert table.seg_offsets.tolist() == sg.SEG_OFFSETS.tolist()
    return table


# ---------------------------------------------------------------------------------------------- seeded entries

@pytest.fixture(scope="module", params=[4, 8])
def entries(request, gpu_device):
    """(K, host arrays of random_timeline, the same on the device, per mode the reference's (pair_dist, totals, pairs, gaps)
    and segment score)."""
    k = request.param
    host = sg.random_timeline(k, sg.SEEDS[k])
    cell, det_dir, count, offsets, dirs, refs = host
    dev = tuple(torch.from_numpy(np.ascontiguousarray(a)).to(gpu_device) for a in host[:5])
    want = {}
    for mode, dd in (("cells", sg.cell_dirs(cell)), ("dirs", det_dir.astype(np.float64))):
        assigned = sg.pair_dist(refs, dd, count, k)
        scored = sg.segment_score(assigned[0], np.diff(offsets).reshape(Q, 13), count, k, sg.SEG_OFFSETS)
        for a in assigned[:2] + scored[:5]:
            a.setflags(write=False)
        want[mode] = (assigned, scored)
    return k, host, dev, want


def _assign(mode, dev, thr=20.0):
    import seld_eval
    cell, det_dir, count, offsets, dirs = dev
    return seld_eval.doa_assign(cell, count, offsets, dirs, thr, det_dir=det_dir if mode == "dirs" else None)


@pytest.mark.parametrize("mode", ["cells", "dirs"])
def test_assignment_equals_the_reference_and_adds_up_to_the_matchers_cost(entries, mode):
    """pair_dist against the restatement: the NaN pattern exactly, the distances within 1e-9 relative; the slots of every
    entry, added in the matcher's row order, are seld_doa_match's cost bit for bit.  No entry of the input has two
    assignments within 1e-9 degrees of each other, so the comparison cannot hinge on a rounding."""
    import seld_eval
    k, host, dev, want = entries
    cell, det_dir, count, offsets, dirs = dev
    (want_pairs, want_totals, pairs, gaps), _ = want[mode]
    assert gaps.min() >= 1e-9, f"near tie of two assignments: {gaps.min()}"
    pair_dist = _assign(mode, dev)
    assert tuple(pair_dist.shape) == (Q, 13, 8) and pair_dist.dtype == torch.float64
    got = pair_dist.cpu().numpy()
    assert np.array_equal(np.isnan(got), np.isnan(want_pairs))
    assert _close(got, want_pairs, 1e-9)
    if mode == "dirs":
        _, cost = seld_eval.doa_match_dirs(det_dir, count, offsets, dirs, 20.0)
    else:
        _, cost = seld_eval.doa_match(cell, count, offsets, dirs, 20.0)
    cost = cost.cpu().numpy()
    sums = np.array([[sg.row_order_sum(got[q, c], pairs[q * 13 + c]) for c in range(13)] for q in range(Q)])
    assert np.array_equal(_bits(sums), _bits(cost))
    assert _close(cost, want_totals, 1e-9)
    n_refs, n_dets = np.diff(host[3]).reshape(Q, 13), host[2]
    assigned = (~np.isnan(got)).sum(-1)
    assert np.array_equal(assigned, np.minimum(n_refs, n_dets))
    both = ((n_refs > n_dets) & (n_dets > 0)).sum(), ((n_refs < n_dets) & (n_refs > 0)).sum()
    assert min(both) > 20                                                # both orientations of the dp
    assert not n_dets[:, 11].any() and n_refs[:, 11].any() and not n_refs[:, 12].any() and n_dets[:, 12].any()
    print(f"K={k} {mode}: {int(assigned.sum())} pairs, smallest gap between two assignments {gaps.min():.3g} degrees")


def test_assignment_on_cell_centres_given_as_directions_is_bit_identical(entries):
    import seld_eval
    k, host, dev, want = entries
    cell, det_dir, count, offsets, dirs = dev
    centres = seld_eval.cell_centre_dirs(cell.clamp(min=0))
    on_centres = seld_eval.doa_assign(None, count, offsets, dirs, 20.0, det_dir=centres)
    assert np.array_equal(_bits(on_centres.cpu().numpy()), _bits(_assign("cells", dev).cpu().numpy()))


def test_assignment_refuses_what_the_matcher_refuses(entries, gpu_device):
    """Nine references, a count above K and a negative count: NaN throughout, the neighbours untouched."""
    import seld_eval
    k, host, dev, want = entries
    cell, det_dir, count, offsets, dirs = dev
    refs = [list(r) for r in host[5]]
    refs[5 * 13 + 3] = [(10 * i - 40, 0) for i in range(9)]
    offs = torch.from_numpy(np.concatenate([[0], np.cumsum([len(r) for r in refs])]).astype(np.int32)).to(gpu_device)
    drs = torch.from_numpy(np.array([d for r in refs for d in r], np.int32).reshape(-1, 2)).to(gpu_device)
    bad_count = count.clone()
    bad_count[6, 4], bad_count[7, 5] = k + 1, -1
    got = seld_eval.doa_assign(cell, bad_count, offs, drs, 20.0).cpu().numpy()
    good = _assign("cells", dev).cpu().numpy()
    refused = np.zeros((Q, 13), bool)
    for q, c in ((5, 3), (6, 4), (7, 5)):
        refused[q, c] = True
        assert np.isnan(got[q, c]).all()
    assert np.array_equal(_bits(got[~refused]), _bits(good[~refused]))
    stats, cost = seld_eval.doa_match(cell, bad_count, offs, drs, 20.0)                         # the matcher's own refusals
    assert (stats.cpu().numpy()[refused][:, 3] == -1).all() and np.isnan(cost.cpu().numpy()[refused]).all()


def test_tie_rule_on_exact_ties(gpu_device):
    """Two identical references and two different detections tie to the bit: slot 0 gets detection 1, slot 1 detection 0
    (masks ascending, candidates ascending, strict <).  Three identical references and two detections (the detections are
    the rows): reference 1 gets detection 0, reference 0 detection 1, reference 2 nothing."""
    import seld_eval
    x0, x1 = 9 * 36 + 16, 10 * 36 + 22                                   # centres (-15, 5) and (45, 15)
    for k in (2, 4):
        cell = np.full((2, 13, k), -1, np.int32)
        count = np.zeros((2, 13), np.int32)
        cell[0, 3, :2], count[0, 3] = (x0, x1), 2
        cell[1, 7, :2], count[1, 7] = (x0, x1), 2
        refs = [[] for _ in range(26)]
        refs[3], refs[13 + 7] = [(10, 0)] * 2, [(10, 0)] * 3
        offsets = np.concatenate([[0], np.cumsum([len(r) for r in refs])]).astype(np.int32)
        dirs = np.array([d for r in refs for d in r], np.int32).reshape(-1, 2)
        want, _, pairs, gaps = sg.pair_dist(refs, sg.cell_dirs(cell), count, k)
        assert gaps[0, 3] == 0.0 and gaps[1, 7] == 0.0                    # exact ties in the restatement
        assert pairs[3] == [(0, 1), (1, 0)] and pairs[13 + 7] == [(1, 0), (0, 1)]
        d0, d1 = (float(ref.angle_deg(10, 0, *ref.cell_centre(x))) for x in (x0, x1))
        assert abs(d1 - d0) > 5.0
        dev = [torch.from_numpy(a).to(gpu_device) for a in (cell, count, offsets, dirs)]
        for det_dir in (None, seld_eval.cell_centre_dirs(dev[0].clamp(min=0))):
            got = seld_eval.doa_assign(dev[0], dev[1], dev[2], dev[3], 20.0, det_dir=det_dir).cpu().numpy()
            assert np.array_equal(np.isnan(got), np.isnan(want)) and _close(got, want, 1e-9)
            assert abs(got[0, 3, 0] - d1) <= 1e-9 * d1 and abs(got[0, 3, 1] - d0) <= 1e-9 * d0
            assert abs(got[1, 7, 1] - d0) <= 1e-9 * d0 and abs(got[1, 7, 0] - d1) <= 1e-9 * d1 and math.isnan(got[1, 7, 2])


# ---------------------------------------------------------------------------------------------- the segment score

@pytest.mark.parametrize("mode", ["cells", "dirs"])
def test_segment_score_equals_the_reference(entries, mode):
    """seld_segment_score on the device's own assignment against the restatement on its own: every integer record exact,
    seg_de / rec_de within 1e-9 relative, two runs bit-identical.  The input keeps every slot average at least 1e-6 degrees
    from the threshold (1e-9 relative of a distance is at most 1.8e-7 degrees), so no count hinges on a rounding."""
    import seld_eval
    k, host, dev, want = entries
    cell, det_dir, count, offsets, dirs = dev
    _, (seg_stats, seg_de, rec_counts, rec_sdi, rec_de, averages) = want[mode]
    margin = float(np.abs(np.array(averages) - sg.THR).min())
    assert margin >= 1e-6, f"a slot average lies {margin} degrees from the threshold"
    pair_dist = _assign(mode, dev)
    one = seld_eval.segment_score(pair_dist, count, k, offsets, _table(), 20.0)
    two = seld_eval.segment_score(pair_dist, count, k, offsets, _table(), 20.0)
    assert [tuple(t.shape) for t in one] == [(5, 13, 8), (5, 13), (3, 13, 11), (3, 3), (3, 13)]
    assert [t.dtype for t in one] == [torch.int32, torch.float64, torch.int64, torch.int64, torch.float64]
    got = [t.cpu().numpy() for t in one]
    assert np.array_equal(got[0], seg_stats) and np.array_equal(got[2], rec_counts) and np.array_equal(got[3], rec_sdi)
    assert _close(got[1], seg_de, 1e-9) and _close(got[4], rec_de, 1e-9)
    for a, b in zip(one, two):
        assert torch.equal(a.view(torch.int64) if a.dtype == torch.float64 else a,
                           b.view(torch.int64) if b.dtype == torch.float64 else b)
    tot = seg_stats.sum((0, 1))
    print(f"K={k} {mode}: Nref {tot[0]} TP {tot[2]} FPs {tot[3]} FP {tot[4]} FN {tot[5]}, margin {margin:.3g} degrees")
    assert tot[2] > 20 and tot[3] > 20 and tot[4] > 20 and tot[5] > 10   # every kind of count occurs
    assert not seg_stats[:, 11, 1].any() and seg_stats[:, 11, 5].sum() == seg_stats[:, 11, 0].sum() > 0
    assert not seg_stats[:, 12, 0].any() and seg_stats[:, 12, 4].sum() == seg_stats[:, 12, 1].sum() > 0


# ---------------------------------------------------------------------------------------------- the jackknife kernel

def test_jackknife_kernel_equals_the_reference(entries):
    """On the rec_* arrays the device produced: every replicate's micro and macro figures within 1e-12 relative (nan-aware),
    row S = the metrics of all recordings, out_class its per-class figures; a single recording works (its one replicate is
    empty: nan, LE 180)."""
    import seld_eval
    k, host, dev, want = entries
    cell, det_dir, count, offsets, dirs = dev
    _, _, rec_counts, rec_sdi, rec_de = seld_eval.segment_score(_assign("cells", dev), count, k, offsets, _table(), 20.0)
    host_rec = rec_counts.cpu().numpy(), rec_sdi.cpu().numpy(), rec_de.cpu().numpy()
    out, out_class = seld_eval.jackknife_score(rec_counts, rec_sdi, rec_de)
    assert tuple(out.shape) == (4, 2, 5) and tuple(out_class.shape) == (13, 5) and out.dtype == torch.float64
    want_out, want_class = sg.jackknife_rows(*host_rec)
    assert _close(out.cpu().numpy(), want_out, 1e-12) and _close(out_class.cpu().numpy(), want_class, 1e-12)
    micro, macro, per_class = sg.metrics(*host_rec, [0, 1, 2])
    assert _close(out[3].cpu().numpy(), np.array([micro, macro]), 1e-12)
    assert not np.isnan(want_out).any() and len({float(v) for v in want_out[:, 1, 4]}) == 4     # the replicates differ
    assert np.isnan(want_class[12, 1]) and want_class[11].tolist() == [0.0, 1.0, 180.0, 0.0, 1.0]
    one, one_class = seld_eval.jackknife_score(rec_counts[:1], rec_sdi[:1], rec_de[:1])
    want_one, want_one_class = sg.jackknife_rows(*(a[:1] for a in host_rec))
    assert tuple(one.shape) == (2, 2, 5)
    assert _close(one.cpu().numpy(), want_one, 1e-12) and _close(one_class.cpu().numpy(), want_one_class, 1e-12)
    assert np.isnan(one[0, 1].cpu().numpy()).all() and float(one[0, 0, 2]) == 180.0


# ---------------------------------------------------------------------------------------------- error returns

def test_error_returns(entries, gpu_device):
    """K = 0, K = 9, a null pointer and S = 0 for the jackknife: each export answers -1 and launches nothing."""
    import seld_eval
    import seld_native
    k, host, dev, want = entries
    cell, det_dir, count, offsets, dirs = dev
    table = _table()
    pair_dist = _assign("cells", dev)
    seg_stats, seg_de, rec_counts, rec_sdi, rec_de = seld_eval.segment_score(pair_dist, count, k, offsets, table, 20.0)
    out, out_class = seld_eval.jackknife_score(rec_counts, rec_sdi, rec_de)
    torch.cuda.synchronize(gpu_device)
    lib = seld_native.load_library()
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    seg_offsets = torch.from_numpy(table.seg_offsets).to(gpu_device)
    blocks = torch.from_numpy(seld_eval.block_table(table)).to(gpu_device)

    def assign(kk=k, cells=cell, counts=count, offs=offsets, drs=dirs, dst=pair_dist, I=18, J=36):
        return lib.seld_doa_assign(p(cells), None, p(counts), kk, p(offs), p(drs), Q, I, J, 20.0, p(dst), None)

    def score(kk=k, pairs=pair_dist, counts=count, offs=offsets, segs=seg_offsets, blk=blocks, stats=seg_stats, n_seg=3):
        return lib.seld_segment_score(p(pairs), p(counts), kk, p(offs), p(segs), p(blk), n_seg, 20.0, p(stats), p(seg_de),
                                      p(rec_counts), p(rec_sdi), p(rec_de), None)

    def jack(counts=rec_counts, sdi=rec_sdi, dst=out, n_seg=3):
        return lib.seld_jackknife_score(p(counts), p(sdi), p(rec_de), n_seg, p(dst), p(out_class), None)

    with torch.cuda.device(gpu_device):
        before = [t.clone() for t in (pair_dist, seg_stats, rec_counts, out)]
        assert assign(kk=0) == -1 and assign(kk=9) == -1 and score(kk=0) == -1 and score(kk=9) == -1
        assert assign(cells=None) == -1 and assign(counts=None) == -1 and assign(offs=None) == -1 and assign(dst=None) == -1
        assert assign(I=0) == -1
        assert score(pairs=None) == -1 and score(segs=None) == -1 and score(blk=None) == -1 and score(stats=None) == -1
        assert score(n_seg=-1) == -1
        assert jack(n_seg=0) == -1 and jack(counts=None) == -1 and jack(sdi=None) == -1 and jack(dst=None) == -1
        assert b"seld_jackknife_score" in lib.seld_last_error()
        assert assign() == 0 and score() == 0 and jack() == 0            # the same calls with nothing wrong
        torch.cuda.synchronize(gpu_device)
    for a, b in zip(before, (pair_dist, seg_stats, rec_counts, out)):
        assert torch.equal(a.view(torch.int64) if a.dtype == torch.float64 else a,
                           b.view(torch.int64) if b.dtype == torch.float64 else b)
    with pytest.raises(seld_native.SeldNativeError):
        seld_eval.doa_assign(cell.cpu(), count.cpu(), offsets.cpu(), dirs.cpu(), 20.0)
    with pytest.raises(ValueError):
        seld_eval.doa_assign(cell, count, offsets[:-1], dirs, 20.0)
    with pytest.raises(ValueError):
        seld_eval.segment_score(pair_dist[:-1], count, k, offsets, table, 20.0)
    with pytest.raises(ValueError):
        seld_eval.jackknife_score(rec_counts, rec_sdi[:2], rec_de)


# ---------------------------------------------------------------------------------------------- end to end

E2E_SEGMENTS = np.array([[0, 113], [113, 90], [203, 118]])      # 321 frames, 7 windows; 23, 18 and 24 meta-frames, 8 blocks
E2E_TOTAL = 321
FIGURES = ("F", "ER", "LE", "LR", "SELD")
COUNTS = ("Nref", "Npred", "TP", "FPs", "FP", "FN", "DE_TP", "DE_FN")


@pytest.fixture(scope="module")
def timeline(gpu_device):
    """(fp32 logits [7, 250, 648, 14] on the device, reference rows per recording).  The references come from the decode at
    0.5: most detections get a reference a few degrees off (three in ten up to 40 degrees per axis off: beyond the
    threshold), some none, plus stray rows."""
    import seld_eval
    logits = torch.from_numpy(ref.planted_logits(E2E_SEGMENTS, 3)).to(gpu_device)
    table = seld_eval.meta_frame_table(E2E_SEGMENTS)
    cells, _, counts = seld_eval.grid_decode(logits, 0, table, 0, len(table), 0.5, 8)
    cells, counts = cells.cpu().numpy(), counts.cpu().numpy()
    rng = np.random.default_rng(8)
    rows = [[], [], []]
    for q in range(len(table)):
        s, m = int(table.segment[q]), int(table.index[q])
        for c in range(13):
            for r in range(int(counts[q, c])):
                if rng.uniform() < 0.85:
                    az, el = ref.cell_centre(cells[q, c, r])
                    spread = 40 if rng.uniform() < 0.3 else 4
                    rows[s].append([m, c, r, int(np.clip(az + rng.integers(-spread, spread + 1), -180, 180)),
                                    int(np.clip(el + rng.integers(-spread, spread + 1), -90, 90))])
        if rng.uniform() < 0.3:
            rows[s].append([m, int(rng.integers(0, 13)), 7, int(rng.integers(-180, 181)), int(rng.integers(-90, 91))])
    return logits, [np.array(r, dtype=np.int64).reshape(-1, 5) for r in rows]


def _dataset(rows, device):
    return SimpleNamespace(segments=E2E_SEGMENTS, metadata_rows=rows, total_frames=E2E_TOTAL, I=18, J=36, device=device)


def _batches(logits):
    return (logits[lo:lo + 3] for lo in range(0, logits.shape[0], 3))


def _same(a, b):
    if isinstance(a, float) and isinstance(b, float) and math.isnan(a) and math.isnan(b):
        return True
    if isinstance(a, list):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(_same(a[k], b[k]) for k in a)
    return a == b


MODES = {"plain": {}, "refine": {"refine": True}, "track": {"track": {"min_len": 1, "max_gap": 1}},
         "track-refine": {"track": {"min_len": 1, "max_gap": 1}, "refine": True}}


@pytest.mark.parametrize("mode", list(MODES))
def test_evaluate_logits_reports_the_segment_metrics_of_the_detections_it_scores(timeline, gpu_device, mode):
    """evaluate_logits(segment=True, jackknife=True): the counts are the restatement's on the detections the main result
    scores (decoded, linked and refined with the public functions evaluate_logits itself calls), the figures and the
    intervals follow from them, n = 3; with the switches off the result has no "segment" key and is otherwise the same."""
    import config
    import seld_eval
    logits, rows = timeline
    ds = _dataset(rows, gpu_device)
    kw = MODES[mode]
    refine = bool(kw.get("refine"))
    off = seld_eval.evaluate_logits(_batches(logits), ds, threshold=0.5, max_peaks=8, **kw)
    on = seld_eval.evaluate_logits(_batches(logits), ds, threshold=0.5, max_peaks=8, segment=True, jackknife=True, **kw)
    assert "segment" not in off and _same({key: v for key, v in on.items() if key != "segment"}, off)
    plain = seld_eval.evaluate_logits(_batches(logits), ds, threshold=0.5, max_peaks=8, segment=True, **kw)
    assert "ci" not in plain["segment"] and _same({key: v for key, v in on["segment"].items() if key != "ci"}, plain["segment"])
    seg = on["segment"]
    # the detections the main result scores
    table = seld_eval.meta_frame_table(E2E_SEGMENTS, E2E_TOTAL)
    decoded = seld_eval.decode(_batches(logits), table, 0.5, 8, device=gpu_device, refine=refine)
    cell, count, det_dir = decoded[0], decoded[2], decoded[4] if refine else None
    if "track" in kw:
        linked = seld_eval.track(cell, count, table, float(config.Config.SELD_TRACK_GATE_DEG), kw["track"]["max_gap"],
                                 kw["track"]["min_len"])
        if refine:
            det_dir = seld_eval.track_dirs(linked[0], linked[2], cell, count, det_dir)
        cell, count = linked[0], linked[2]
    cell, count = cell.cpu().numpy(), count.cpu().numpy()
    det_dirs = det_dir.cpu().numpy().astype(np.float64) if refine else sg.cell_dirs(cell)
    offsets, dirs = seld_eval.reference_table(table, rows)
    refs = [dirs[offsets[i]:offsets[i + 1]].tolist() for i in range(len(table) * 13)]
    pairs, _, _, gaps = sg.pair_dist(refs, det_dirs, count, 8)
    scored = sg.segment_score(pairs, np.diff(offsets).reshape(-1, 13), count, 8, table.seg_offsets)
    seg_stats, _, rec_counts, rec_sdi, rec_de, averages = scored
    margin = float(np.abs(np.array(averages) - sg.THR).min())
    print(f"{mode}: counts {seg['counts']}, macro {seg['macro']}, smallest gap {gaps.min():.3g}, margin {margin:.3g} degrees")
    # nothing of the input hinges on a rounding (an exact tie, of duplicate rows, is resolved by the stated rule on both sides)
    assert not ((gaps > 0.0) & (gaps < 1e-9)).any() and margin >= 1e-6
    totals = rec_counts.sum(0)
    for i, name in enumerate(COUNTS + ("S", "D", "I")):
        assert seg["per_class"][name] == totals[:, i].tolist(), name
    for i, name in enumerate(COUNTS):
        assert seg["counts"][name] == int(totals[:, i].sum()), name
    assert [seg["counts"][name] for name in ("S", "D", "I")] == rec_sdi.sum(0).tolist()
    assert seg["blocks"] == 8 and seg["recordings"] == 3 and seg["block_seconds"] == 1.0
    assert seg["classes"] == [c for c in range(13) if totals[c, 0] > 0] and len(seg["classes"]) >= 10
    assert seg["counts"]["TP"] > 30 and seg["counts"]["FPs"] > 3 and seg["counts"]["FN"] > 3
    want_out, want_class = sg.jackknife_rows(rec_counts, rec_sdi, rec_de)
    for a, avg in enumerate(("micro", "macro")):
        assert set(seg[avg]) == set(FIGURES)
        assert _close([seg[avg][name] for name in FIGURES], want_out[3, a], 1e-9), avg
        for i, name in enumerate(FIGURES):
            ci = seg["ci"][avg][name]
            assert set(ci) == {"estimate", "bias", "se", "low", "high", "n"} and ci["n"] == 3
            want = sg.jackknife(want_out[:3, a, i], want_out[3, a, i], sg.T975[2])
            got = [ci[key] for key in ("estimate", "bias", "se", "low", "high")]
            # each is a combination of the four figures (held to 1e-9 relative) with coefficients that sum to less than
            # 2 (n - 1) + 2 t sqrt(n - 1) < 20 in absolute value
            bound = 20 * 1e-9 * np.abs(want_out[:, a, i]).max()
            assert all(abs(g - w) <= bound for g, w in zip(got, want[:5])), (avg, name, got, want)
            assert ci["low"] <= ci["estimate"] <= ci["high"]
    assert _close(np.array([seg["per_class"][name] for name in FIGURES]).T, want_class, 1e-9)
    assert 0.0 < seg["macro"]["SELD"] < 1.0 and seg["macro"]["F"] != seg["micro"]["F"]
