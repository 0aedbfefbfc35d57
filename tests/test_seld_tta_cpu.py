"""CPU checks of test-time augmentation in the SELD evaluation: the pattern-list parser and the
parameter rows, the float64 restatement (tests/seld_tta_ref.py) on exact permuted copies, the planted cases the GPU test
uses, the compiler's resource report of csrc/seld_tta.hip, and the refusal to run without a device timeline."""
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import seld_eval_ref as ref
import seld_tta_ref as tta

CSRC = Path(__file__).resolve().parent.parent / "sound-event-localization-detection_amd" / "csrc"
# detections of the float64 restatement at threshold 0.5, K = 1 / 4 / 8
DETECTIONS = {"bf16-all": (38, 58, 63), "fp32-three": (42, 59, 62), "fp32-one": (46, 66, 73)}


def test_tta_patterns_parsing():
    from seld_augment import tta_patterns
    for off in (None, (), [], 0, False, ""):
        assert tta_patterns(off) == ()
    assert tta_patterns("all") == tuple(range(16)) and tta_patterns(" ALL ") == tuple(range(16))
    assert tta_patterns("0,2,9") == (0, 2, 9) and tta_patterns(" 9, 2 ,0") == (9, 2, 0)      # order kept
    assert tta_patterns([3, 1, 15]) == (3, 1, 15) and tta_patterns((5,)) == (5,) and tta_patterns("7") == (7,)
    assert tta_patterns(np.array([4, 0], dtype=np.int64)) == (4, 0) and tta_patterns(range(16)) == tuple(range(16))
    assert tta_patterns(5) == (5,)
    assert all(type(p) is int for p in tta_patterns(np.array([4, 0])))
    for bad in ("0,16", "-1", [16], [0, 0], "2,2", "x", "1,,2", [1.5], ["1"], True, -1, list(range(16)) + [0]):
        with pytest.raises(ValueError):
            tta_patterns(bad)


def test_tta_rows():
    import seld_augment
    rows = seld_augment.tta_rows(11, 5)
    assert rows.dtype == np.int32 and rows.shape == (5, seld_augment.PARAM_INTS)
    assert (rows[:, 0] == 11).all() and not rows[:, 1:].any()
    assert np.array_equal(seld_augment.tta_rows(0, 3), seld_augment.identity_rows(3))
    assert seld_augment.tta_rows(4, 0).shape == (0, seld_augment.PARAM_INTS)
    for bad in (-1, 16):
        with pytest.raises(ValueError):
            seld_augment.tta_rows(bad, 2)


def test_check_tta_names_the_feature_set():
    import seld_augment
    seld_augment.check_tta((0, 3), "logmel", 4)
    seld_augment.check_tta((0, 3), "logmel_iv", 7)
    seld_augment.check_tta((), "logmel_gcc", 10)                      # off: nothing to refuse
    for feature_set, channels in (("logmel_gcc", 10), ("logmel", 8), ("logmel_iv", 4)):
        with pytest.raises(ValueError, match="microphone array"):
            seld_augment.check_tta((0, 3), feature_set, channels)


def test_restatement_of_exact_permuted_copies_is_the_plain_decode():
    """Without the stacks' noise every un-permuted stack IS the base, so the averaged map equals the plain one."""
    import seld_augment
    base = ref.planted_logits(tta.SEG, 2234)
    want = ref.decode_probs(base, tta.SEG, tta.TOTAL)
    patterns = (2, 6, 11, 0, 13)
    x = np.stack([base[:, :, seld_augment.cell_source(p), :] for p in patterns])
    assert np.abs(tta.decode_probs_tta(x, patterns) - want).max() <= 1e-12
    # and the direction matters: cell_source for cell_dest is caught for a quarter turn without mirror
    wrong = ref.decode_probs(x[0][:, :, seld_augment.cell_source(2), :], tta.SEG, tta.TOTAL)
    assert np.abs(wrong - want).max() > 0.1


@pytest.mark.parametrize("name", list(tta.CASES))
def test_planted_cases_have_few_near_ties(name):
    """What the GPU comparison may exclude, from the restatement alone: at most 1 % of the 286 entries (measured: none),
    and the detection counts the inputs were designed to give (K = 1 and 4 truncate)."""
    _, patterns, x, want = tta.case(name)
    assert x.shape == (len(patterns), 3, 250, 648, 14) and want.shape == (22, 648, 13)
    assert any(p in (2, 3, 6, 7) for p in patterns)
    for k, count in zip((1, 4, 8), DETECTIONS[name]):
        dets, near = ref.decode_detections(want, tta.THRESHOLD, k)
        assert near.size == 286 and float(near.mean()) <= 0.01, (k, int(near.sum()))
        assert sum(len(c) for row in dets for c in row) == count, k


def test_tta_kernels_do_not_spill():
    """The compiler's own resource report of csrc/seld_tta.hip: both instantiations without scratch and with no more LDS
    than the plain decode kernels of csrc/seld_eval.hip (one staged row)."""
    from hip_resources import report
    got, plain = report(CSRC / "seld_tta.hip"), report(CSRC / "seld_eval.hip")
    print(got)
    kernels = {k: v for k, v in got.items() if "tta_decode_kernel" in k}
    assert len(kernels) == 2 and len(got) == 2, sorted(got)
    assert not any("grid_decode_kernel" in k for k in got)
    assert all(v["scratch"] == 0 for v in got.values()), got
    for bf16 in ("ILb1E", "ILb0E"):
        mine = [v for k, v in kernels.items() if bf16 in k]
        theirs = [v for k, v in plain.items() if "grid_decode_kernel" in k and bf16 in k]
        assert len(mine) == 1 and len(theirs) == 1
        assert mine[0]["lds"] <= theirs[0]["lds"], (mine, theirs)
    assert sorted(v["lds"] for v in kernels.values()) == [33696, 36288]


def test_timeline_logits_with_patterns_needs_the_device_timeline():
    """No CPU fallback: a dataset without spec_tm (keep_on_device=False), or a CPU device, raises before any window is
    gathered -- at the call, not at the first batch -- while the same call without patterns is still a generator."""
    import trainer

    class NoTimeline:
        spec_tm = None

        def __len__(self):
            return 4

        def device_batch(self, *a, **k):
            raise AssertionError("must not be reached")

    model = SimpleNamespace()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        trainer.timeline_logits(model, NoTimeline(), 2, torch.device("cuda", 0), patterns=(0, 2))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        trainer.timeline_logits(model, NoTimeline(), 2, torch.device("cpu"), patterns="all")
    with pytest.raises(ValueError):
        trainer.timeline_logits(model, NoTimeline(), 2, torch.device("cpu"), patterns=(0, 0))
    plain = trainer.timeline_logits(model, NoTimeline(), 2, torch.device("cpu"), patterns=())
    assert hasattr(plain, "__next__")


def test_decode_argument_errors_need_no_gpu():
    import seld_eval
    from seld_native import SeldNativeError
    table = seld_eval.meta_frame_table(tta.SEG, tta.TOTAL)
    with pytest.raises(SeldNativeError):                                          # no CPU fallback
        seld_eval.grid_decode_tta(torch.zeros((1, 3, 250, 648, 14)), (0,), 0, table, 0, 22, 0.5, 4)
    for k in (0, 9):
        with pytest.raises(ValueError):
            seld_eval.decode(iter(()), table, 0.5, k, patterns=(0, 2))
