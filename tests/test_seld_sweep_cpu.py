"""CPU checks of the threshold sweep: the prefix property on the float64 restatement of the decode,
the host side of seld_eval (best-threshold selection, the thresholds file, the sweep spelling, argument conflicts, fp32
rounding, apply_thresholds -- framework ops, so it runs here), and the compiler's resource report of the new kernels."""
import json
import math
import re
import warnings
from pathlib import Path

import numpy as np
import pytest
import torch

import seld_eval_ref as ref
import seld_sweep_ref as sref

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "sound-event-localization-detection_amd" / "csrc"
NAN = float("nan")


# ---------------------------------------------------------------------------------------------- the prefix property

@pytest.fixture(scope="module")
def planted_probs():
    probs = ref.decode_probs(ref.planted_logits(sref.SEGMENTS, sref.SEED), sref.SEGMENTS, sref.TOTAL)
    probs.setflags(write=False)
    return probs


@pytest.mark.parametrize("k", [1, 4, 8])
def test_detections_at_a_threshold_are_a_prefix_of_those_at_a_lower_one(planted_probs, k):
    """decode_detections(P, t, K) is decode_detections(P, t_min, K) cut at score >= t, for every (q, c) and every t of
    the grid; the grid's rows are not all the same."""
    low, _ = ref.decode_detections(planted_probs, min(sref.GRID), k)
    totals = []
    for t in sref.GRID:
        got, _ = ref.decode_detections(planted_probs, t, k)
        assert got == sref.truncate(low, planted_probs, t), t
        totals.append(sum(len(cells) for row in got for cells in row))
    print(f"K={k}: detections per threshold {totals}")
    assert len(set(totals)) >= 3
    assert totals == sorted(totals, reverse=True)


def test_reference_prefix_tables_and_rows_agree():
    """The restatement against itself on a hand case: two references, three detections (the second a duplicate cell far
    from both): the table's entry at each prefix length is the matcher's answer, a threshold's row gathers it."""
    refs = [[] for _ in range(13)]
    refs[2] = [(5, 5), (105, 5)]
    cells = np.full((1, 13, 4), -1, np.int64)
    cells[0, 2, :3] = [9 * 36 + 18, 0, 9 * 36 + 28]                     # centres (5, 5), (-175, -85), (105, 5)
    score = np.zeros((1, 13, 4), np.float32)
    score[0, 2, :3] = [0.9, 0.5, 0.3]
    count = np.zeros((1, 13), np.int64)
    count[0, 2] = 3
    ptp, pcost = sref.prefix_tables(refs, cells, count, 4)
    assert ptp[0, 2].tolist() == [0, 1, 1, 2, 2]
    assert pcost[0, 2, 1] == 0.0 and pcost[0, 2, 3] == 0.0 and pcost[0, 2, 2] > 90.0
    rows = sref.sweep_metrics(refs, cells, score, count, [0.2, 0.4, 0.6, 0.95])
    assert [(r["TP"], r["FP"], r["FN"]) for r in rows] == [(2, 1, 0), (1, 1, 1), (1, 0, 1), (0, 0, 2)]


# ---------------------------------------------------------------------------------------------- apply_thresholds

def test_apply_thresholds_keeps_the_leading_detections_and_restores_the_conventions():
    import seld_eval
    rng = np.random.default_rng(11)
    q, k = 9, 4
    count = rng.integers(0, k + 1, size=(q, 13)).astype(np.int32)
    score = np.sort(rng.uniform(0.05, 1.0, size=(q, 13, k)).astype(np.float32), axis=-1)[..., ::-1].copy()
    score[0, 0] = [0.5, 0.5, 0.25, 0.25]                               # scores exactly at a threshold are kept
    count[0, 0] = 4
    rank = np.arange(k)
    valid = rank < count[..., None]
    score = np.where(valid, score, 0.0).astype(np.float32)
    cell = np.where(valid, rng.integers(0, 648, size=(q, 13, k)), -1).astype(np.int32)
    dirs = np.where(valid[..., None], rng.uniform(-90, 90, size=(q, 13, k, 2)), 0.0).astype(np.float32)
    thr = [0.5 if c == 0 else float(np.float32(0.1 + 0.06 * c)) for c in range(13)]
    got = seld_eval.apply_thresholds(torch.from_numpy(cell), torch.from_numpy(score), torch.from_numpy(count), thr,
                                     torch.from_numpy(dirs))
    got = [t.numpy() for t in got]
    assert got[2].dtype == np.int32 and got[2][0, 0] == 2
    for qi in range(q):
        for c in range(13):
            n = sref.leading(score[qi, c, :count[qi, c]], thr[c])
            assert got[2][qi, c] == n
            assert np.array_equal(got[0][qi, c, :n], cell[qi, c, :n]) and (got[0][qi, c, n:] == -1).all()
            assert np.array_equal(got[1][qi, c, :n], score[qi, c, :n]) and (got[1][qi, c, n:] == 0).all()
            assert np.array_equal(got[3][qi, c, :n], dirs[qi, c, :n]) and (got[3][qi, c, n:] == 0).all()
    assert len(seld_eval.apply_thresholds(torch.from_numpy(cell), torch.from_numpy(score), torch.from_numpy(count), thr)) == 3
    with pytest.raises(ValueError):
        seld_eval.apply_thresholds(torch.from_numpy(cell), torch.from_numpy(score), torch.from_numpy(count), [0.5] * 12)


# ---------------------------------------------------------------------------------------------- best thresholds

def _pc(rows):
    """rows: per threshold a {class: value} -> [T][13] with the other classes 0."""
    return [[row.get(c, 0.0) for c in range(13)] for row in rows]


def test_best_is_the_highest_f20():
    import seld_eval
    t = [0.1, 0.2, 0.3]
    best = seld_eval.select_best(t, [0.4, 0.7, 0.6], [0.9, 0.5, 0.6], _pc([{}, {}, {}]), _pc([{}, {}, {}]))
    assert best["global"] == 0.2 and best["per_class"] == [0.2] * 13      # no class has references


def test_best_ties_go_to_the_lower_er20_then_to_the_lower_threshold():
    import seld_eval
    t = [0.1, 0.2, 0.3, 0.4]
    none = _pc([{}] * 4)
    assert seld_eval.select_best(t, [0.7, 0.7, 0.7, 0.1], [0.5, 0.4, 0.45, 0.0], none, none)["global"] == 0.2
    assert seld_eval.select_best(t, [0.7, 0.7, 0.7, 0.1], [0.5, 0.4, 0.4, 0.0], none, none)["global"] == 0.2
    assert seld_eval.select_best(t, [0.7, 0.7, 0.2, 0.1], [NAN, NAN, 0.1, 0.0], none, none)["global"] == 0.1
    assert seld_eval.select_best(t, [0.7, 0.7, 0.2, 0.1], [NAN, 3.0, 0.1, 0.0], none, none)["global"] == 0.2


def test_a_nan_f20_never_wins_and_all_nan_is_none():
    import seld_eval
    t = [0.1, 0.2, 0.3]
    none = _pc([{}] * 3)
    assert seld_eval.select_best(t, [NAN, 0.0, NAN], [0.0, 9.0, 0.0], none, none)["global"] == 0.2
    best = seld_eval.select_best(t, [NAN, NAN, NAN], [NAN, NAN, NAN], none, none)
    assert best["global"] is None and best["per_class"] == [None] * 13


def test_per_class_best_and_a_class_without_references():
    import seld_eval
    t = [0.1, 0.2, 0.3]
    f20_c = _pc([{0: 0.2, 5: 0.9, 7: NAN}, {0: 0.8, 5: 0.9, 7: NAN}, {0: 0.8, 5: 0.1, 7: NAN}])
    n_c = _pc([{0: 4, 5: 2}, {0: 4, 5: 2}, {0: 4, 5: 2}])
    best = seld_eval.select_best(t, [0.3, 0.5, 0.6], [0.9, 0.6, 0.7], f20_c, n_c)
    assert best["global"] == 0.3
    assert best["per_class"][0] == 0.2          # tie between 0.2 and 0.3 on the class's F20: the lower ER20
    assert best["per_class"][5] == 0.2          # tie between 0.1 and 0.2: ER20 0.9 against 0.6
    assert best["per_class"][7] == 0.3          # no references: the global value
    assert all(best["per_class"][c] == 0.3 for c in (1, 2, 3, 4, 6, 8, 9, 10, 11, 12))


# ---------------------------------------------------------------------------------------------- the sweep spelling

def test_sweep_parser():
    import seld_eval
    f32 = lambda v: float(np.float32(v))
    got = seld_eval.parse_sweep("0.05:0.95:0.05")
    assert len(got) == 19 and got == tuple(f32(round(0.05 * i, 12)) for i in range(1, 20))
    assert seld_eval.parse_sweep("0.1:0.3:0.1") == (f32(0.1), f32(0.2), f32(0.3))      # inclusive despite 0.1 * 3 > 0.3
    assert seld_eval.parse_sweep("0.2:0.2:0.5") == (f32(0.2),)
    assert seld_eval.parse_sweep("0.5, 0.1,0.25") == (f32(0.1), 0.25, 0.5)
    assert seld_eval.parse_sweep([0.9, 0.3]) == (f32(0.3), f32(0.9))
    assert seld_eval.parse_sweep(None) == () and seld_eval.parse_sweep(()) == () and seld_eval.parse_sweep(" ") == ()
    assert len(seld_eval.parse_sweep("0.01:0.64:0.01")) == 64
    for bad in ("0.1:0.5", "0.5:0.1:0.1", "0.1:0.5:0", "0.1:0.5:-0.1", "a,b", "0.1:0.5:0.1:3", [0.0, 0.5], [0.5, 1.5],
                [0.5, 0.5], [0.3, 0.3 + 1e-10], "0.01:0.65:0.01", [-0.1]):
        with pytest.raises(ValueError):
            seld_eval.parse_sweep(bad)


def test_thresholds_are_rounded_to_fp32_once():
    """What the host hands on is exactly representable in fp32, so the decode (a float argument) and the sweep kernel (a
    float array) compare against the same number."""
    import seld_eval
    for v in seld_eval.parse_sweep("0.05:0.95:0.05") + tuple(seld_eval.class_threshold_vector([0.1 + 0.01 * c for c in range(13)])):
        assert v == float(np.float32(v))
    assert seld_eval.parse_sweep([0.1])[0] != 0.1 and seld_eval.parse_sweep([0.1])[0] == float(np.float32(0.1))
    with pytest.raises(ValueError):                                      # two spellings of one fp32 number
        seld_eval.parse_sweep([0.1, float(np.float32(0.1))])


def test_config_defaults_are_off():
    import config
    import seld_eval
    assert config.Config.SELD_SWEEP_THRESHOLDS == () and config.Config.SELD_CLASS_THRESHOLDS is None
    assert config.Config.SELD_THRESHOLDS_OUT is None
    assert seld_eval.sweep_setting(None) == () and seld_eval.class_thresholds_setting(None) is None


# ---------------------------------------------------------------------------------------------- the thresholds file

def _swept():
    none = [[0] * 13] * 3
    return {"thresholds": [0.25, 0.5, 0.75], "F20": [0.5, 0.75, NAN], "ER20": [0.5, 0.25, NAN],
            "best": {"global": 0.5, "per_class": [0.5] * 12 + [0.25]}, "per_class": {"N": none}}


def test_thresholds_file_round_trip(tmp_path):
    import seld_eval
    path = seld_eval.write_thresholds(tmp_path / "sub" / "thresholds.json", _swept(), 4, 20.0, (0, 9), True,
                                      {"gate_deg": 20.0, "max_gap": 2, "min_len": 3, "tracks": 7})
    doc = json.loads(path.read_text())                                   # plain JSON: nan written as null
    assert set(doc) == {"version", "global", "per_class", "max_peaks", "doa_threshold_deg", "tta_patterns", "refine",
                        "tracking", "grid"}
    assert doc["grid"] == {"thresholds": [0.25, 0.5, 0.75], "F20": [0.5, 0.75, None], "ER20": [0.5, 0.25, None]}
    assert doc["tracking"] == {"gate_deg": 20.0, "max_gap": 2, "min_len": 3}
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        got = seld_eval.load_thresholds(path, max_peaks=4, tta_patterns=(0, 9), refine=True)
        assert seld_eval.load_thresholds(path)["per_class"] == got["per_class"]
    assert got["version"] == 1 and got["global"] == 0.5 and got["per_class"] == [0.5] * 12 + [0.25]
    assert got["max_peaks"] == 4 and got["doa_threshold_deg"] == 20.0 and got["tta_patterns"] == [0, 9]
    assert seld_eval.class_thresholds_setting(str(path), 4, (0, 9), True) == got["per_class"]
    for other in ({"max_peaks": 8}, {"tta_patterns": ()}, {"refine": False}):
        with pytest.warns(UserWarning, match=next(iter(other))):
            seld_eval.load_thresholds(path, **{"max_peaks": 4, "tta_patterns": (0, 9), "refine": True, **other})
    swept = _swept()
    swept["best"] = {"global": None, "per_class": [None] * 13}
    with pytest.raises(ValueError):
        seld_eval.write_thresholds(tmp_path / "none.json", swept, 4, 20.0)


def test_thresholds_file_validation(tmp_path):
    import seld_eval
    good = json.loads(seld_eval.write_thresholds(tmp_path / "good.json", _swept(), 4, 20.0).read_text())
    bad = tmp_path / "bad.json"
    with pytest.raises(ValueError):
        seld_eval.load_thresholds(tmp_path / "absent.json")
    bad.write_text("{ not json")
    with pytest.raises(ValueError):
        seld_eval.load_thresholds(bad)
    cases = [{"version": 2}, {"version": None}, {"global": 0.0}, {"global": 1.5}, {"global": "0.5"}, {"global": True},
             {"per_class": [0.5] * 12}, {"per_class": [0.5] * 12 + [0.0]}, {"per_class": [0.5] * 12 + ["x"]},
             {"per_class": 0.5}]
    for change in cases:
        bad.write_text(json.dumps({**good, **change}))
        with pytest.raises(ValueError):
            seld_eval.load_thresholds(bad)
    for key in ("global", "per_class", "max_peaks", "tta_patterns", "refine", "doa_threshold_deg"):
        bad.write_text(json.dumps({k: v for k, v in good.items() if k != key}))
        with pytest.raises(ValueError, match=key):
            seld_eval.load_thresholds(bad)
    bad.write_text(json.dumps([1, 2]))
    with pytest.raises(ValueError):
        seld_eval.load_thresholds(bad)


# ---------------------------------------------------------------------------------------------- argument conflicts

def test_argument_conflicts_raise_before_anything_runs(tmp_path):
    import seld_eval
    with pytest.raises(ValueError, match="not both"):
        seld_eval.evaluate_logits(iter(()), None, threshold=0.5, class_thresholds=[0.5] * 13)
    with pytest.raises(ValueError, match="needs a sweep"):
        seld_eval.evaluate_logits(iter(()), None, thresholds_out=tmp_path / "t.json")
    with pytest.raises(ValueError):
        seld_eval.evaluate_logits(iter(()), None, class_thresholds=[0.5] * 5)
    with pytest.raises(ValueError):
        seld_eval.evaluate_logits(iter(()), None, sweep="0.5:0.1:0.1")
    with pytest.raises(ValueError):
        seld_eval.evaluate_logits(iter(()), None, class_thresholds=tmp_path / "absent.json")
    with pytest.raises(ValueError):
        seld_eval.sweep(None, None, None, None, None, (), 20.0)
    assert not (tmp_path / "t.json").exists()


def test_infer_cli_takes_a_thresholds_file():
    import infer
    args = infer.parse_args(["--checkpoint", "c.pth", "--out-dir", "out", "--thresholds", "t.json", "a.wav"])
    assert args.thresholds == "t.json"
    assert infer.parse_args(["--checkpoint", "c.pth", "--out-dir", "out", "a.wav"]).thresholds is None


def test_evaluate_seld_takes_the_sweep_arguments():
    import inspect
    import seld_eval
    import trainer
    for fn in (trainer.evaluate_seld, seld_eval.evaluate_logits):
        params = inspect.signature(fn).parameters
        assert all(params[name].default is None for name in ("sweep", "class_thresholds", "thresholds_out"))


# ---------------------------------------------------------------------------------------------- the kernels' resources

def test_sweep_kernels_do_not_spill():
    """The compiler's own resource report of the sweep kernels (both prefix instantiations and the score kernel) shows
    no scratch."""
    import hip_resources
    found = {k: v["scratch"] for k, v in hip_resources.report(CSRC / "seld_sweep.hip").items()}
    assert len([k for k in found if "doa_match_prefix_kernel" in k]) == 2 and any("sweep_score_kernel" in k for k in found)
    assert all(v == 0 for v in found.values()), found


def test_header_binding_and_library_agree_on_the_sweep_exports():
    import ctypes
    import seld_native
    header = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "seld_hip.h").read_text(), flags=re.S)
    lib = seld_native.load_library()
    for name in ("seld_doa_match_prefix", "seld_sweep_score"):
        proto = re.search(rf"int {name}\((.*?)\);", header, flags=re.S)
        assert proto, f"{name} is not declared in include/seld_hip.h"
        assert len(getattr(lib, name).argtypes) == len(proto.group(1).split(","))
        assert hasattr(ctypes.CDLL(str(seld_native.LIB_PATH)), name)
