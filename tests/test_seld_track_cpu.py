"""CPU checks of the track linking contract: the product's distance table against the restatement's,
hand cases on the restatement (tests/seld_track_ref.py), the C ABI's three descriptions of seld_track_link, and the
compiler's resource report of csrc/seld_track.hip.  No GPU."""
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import seld_track_ref as tref

ROOT = Path(__file__).resolve().parent.parent
PKG = ROOT / "sound-event-localization-detection_amd"
J = 36


def cell(i, j):
    return i * J + j % J


def run(frames, gate_deg=20.0, max_gap=2, min_len=1):
    return tref.link_chain(frames, tref.distance_table(), int(np.rint(1000 * gate_deg)), max_gap, min_len)


def ids_at(out, m):
    return {c: tid for tid, c in out[m]}


def test_product_distance_table_equals_the_restatement():
    import seld_eval
    got = seld_eval.track_distance_table(18, 36).numpy()
    want = tref.distance_table(18, 36)
    assert got.dtype == np.int32 and got.shape == (18, 18, 36)
    assert np.array_equal(got, want)
    assert int((want == 20000).sum()) == 36                    # (i, i +- 2, 0) and nothing else
    assert (want[np.arange(18), np.arange(18), 0] == 0).all()
    # the table is indexed by the azimuth difference: every pair of cells against the direct formula
    import seld_eval_ref as ref
    rng = np.random.default_rng(0)
    a, b = rng.integers(0, 648, 2000), rng.integers(0, 648, 2000)
    d = ref.angle_deg(*ref.cell_centre(a), *ref.cell_centre(b))
    assert [tref.dist(want, int(x), int(y)) for x, y in zip(a, b)] == np.rint(1000 * d).astype(int).tolist()
    assert seld_eval.track_distance_table(18, 36) is seld_eval.track_distance_table(18, 36)       # cached


def test_two_sources_that_swap_rank_keep_their_ids():
    a = [cell(9, j) for j in (5, 5, 6, 6, 7, 7)]
    b = [cell(4, j) for j in (30, 31, 31, 32, 32, 33)]
    frames = [[x, y] if m % 2 == 0 else [y, x] for m, (x, y) in enumerate(zip(a, b))]
    out, tracks, _ = run(frames)
    for m in range(6):
        assert ids_at(out, m) == {a[m]: 0, b[m]: 1}
    assert tracks == [(0, 5, 6, 1), (0, 5, 6, 1)]


def test_two_frame_dropout_is_filled_at_gap_2_and_splits_at_gap_1():
    x = cell(9, 10)
    frames = [[x], [x], [], [], [x], [x]]
    out, tracks, stats = run(frames, max_gap=2)
    assert [row for row in out] == [[(0, x)]] * 6 and tracks == [(0, 5, 4, 1)] and stats["fills"] == 2
    out, tracks, stats = run(frames, max_gap=1)
    assert out == [[(0, x)], [(0, x)], [], [], [(1, x)], [(1, x)]]
    assert tracks == [(0, 1, 2, 1), (4, 5, 2, 1)] and stats["fills"] == 0
    # the fill carries the cell before the update
    y = cell(9, 11)
    out, _, _ = run([[x], [], [y]], max_gap=1)
    assert out == [[(0, x)], [(0, x)], [(0, y)]]


def test_one_frame_clutter_is_dropped_at_min_len_2():
    x, clutter = cell(9, 10), cell(2, 30)
    out, tracks, stats = run([[x], [x, clutter], [x]], max_gap=0, min_len=2)
    assert out == [[(0, x)], [(0, x)], [(0, x)]]
    assert tracks == [(0, 2, 3, 1), (1, 1, 1, 0)] and stats["removed"] == 1
    out, _, _ = run([[x], [x, clutter], [x]], max_gap=0, min_len=1)
    assert out[1] == [(0, x), (1, clutter)]


def test_gate_is_inclusive_to_the_milli_degree():
    a, b = cell(7, 12), cell(9, 12)                             # 20 degrees apart along a meridian
    assert tref.dist(tref.distance_table(), a, b) == 20000
    out, tracks, stats = run([[a], [b]], gate_deg=20.0)
    assert out == [[(0, a)], [(0, b)]] and stats["gate_exact"] == 1
    out, tracks, _ = run([[a], [b]], gate_deg=19.999)
    assert out == [[(0, a)], [(1, b)]] and len(tracks) == 2


def test_azimuth_wraps():
    a, b = cell(9, 35), cell(9, 0)
    out, tracks, _ = run([[a], [b]], gate_deg=15.0)
    assert out == [[(0, a)], [(0, b)]] and tracks == [(0, 1, 2, 1)]
    lo, hi = cell(0, 0), cell(17, 0)                            # elevation does not
    out, tracks, _ = run([[lo], [hi]], gate_deg=15.0)
    assert len(tracks) == 2


def test_ninth_track_evicts_the_oldest():
    cells = [cell(2 + 4 * (n // 4), 9 * (n % 4)) for n in range(8)]          # far apart: nothing links across
    frames = [[cells[0]], cells[1:], [], [cell(16, 4)]]
    out, tracks, stats = run(frames, gate_deg=5.0, max_gap=3)
    assert stats["evictions"] == 1
    assert tracks[0] == (0, 0, 1, 1) and tracks[8] == (3, 3, 1, 1)          # track 0, last seen longest ago, ended
    assert out[3] == [(8, cell(16, 4))]
    # lowest slot index on equal last_m: with all eight born in one frame, slot 0's track goes
    out, tracks, stats = run([cells, [], [cell(16, 4)]], gate_deg=5.0, max_gap=3)
    assert stats["evictions"] == 1 and len(tracks) == 9
    out2, _, _ = run([cells, [], [cell(16, 4)], cells], gate_deg=5.0, max_gap=3)
    assert {tid for tid, _ in out2[3]} == {1, 2, 3, 4, 5, 6, 7, 9}          # cells[0] starts anew, the others were filled


def test_generator_meets_the_gpu_tests_conditions():
    """The four settings of the GPU test, on the restatement alone (the GPU test asserts the same before it compares)."""
    for k, gap, min_len, gate, seed in tref.GPU_SETTINGS:
        det_cell, det_count, seg = tref.synthetic_detections(tref.GPU_SEGMENTS, k, seed)
        *_, stats = tref.track(det_cell, det_count, seg, tref.distance_table(), int(np.rint(1000 * gate)), gap, min_len)
        print(k, gap, min_len, gate, stats)
        tref.assert_exercised(stats, k, gap, min_len, gate)


def test_header_binding_and_library_agree_on_seld_track_link():
    import ctypes
    import seld_native
    header = (ROOT / "include" / "seld_hip.h").read_text()
    proto = re.search(r"int seld_track_link\((.*?)\);", re.sub(r"/\*.*?\*/", "", header, flags=re.S), flags=re.S)
    assert proto, "seld_track_link is not declared in include/seld_hip.h"
    params = [p.strip() for p in proto.group(1).split(",")]
    lib = seld_native.load_library()
    argtypes = lib.seld_track_link.argtypes
    assert len(argtypes) == len(params) == 18
    for p, a in zip(params, argtypes):
        want = ctypes.c_void_p if "*" in p else (ctypes.c_int64 if p.startswith("int64_t") else ctypes.c_int)
        assert a is want, (p, a)
    assert hasattr(ctypes.CDLL(str(PKG / "libseld_hip.so")), "seld_track_link")


def test_track_kernels_use_no_scratch():
    csrc = PKG / "csrc"
    run_ = subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", f"-I{ROOT / 'include'}",
                           "-Rpass-analysis=kernel-resource-usage", "-c", str(csrc / "seld_track.hip"), "-o", "/dev/null"],
                          capture_output=True, text=True)
    assert run_.returncode == 0, run_.stderr[-2000:]
    found, current = {}, None
    for line in run_.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            current = m.group(1)
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
        if m and current:
            found[current] = int(m.group(1))
    assert any("track_chain_kernel" in k for k in found) and any("track_compact_kernel" in k for k in found), sorted(found)
    assert all(v == 0 for v in found.values()), found


def test_track_settings_read_config_and_overrides():
    import seld_eval
    from config import Config
    assert Config.SELD_TRACK is False and seld_eval.track_settings(None) is None and seld_eval.track_settings(False) is None
    assert seld_eval.track_settings(True) == {"gate_deg": 20.0, "max_gap": 2, "min_len": 3}
    assert seld_eval.track_settings({"max_gap": 0}) == {"gate_deg": 20.0, "max_gap": 0, "min_len": 3}
    with pytest.raises(ValueError):
        seld_eval.track_settings({"gap": 1})


def test_track_refuses_cpu_tensors():
    import torch
    import seld_eval
    from seld_native import SeldNativeError
    table = seld_eval.meta_frame_table(np.array([[0, 50]]))
    with pytest.raises(SeldNativeError):
        seld_eval.track(torch.zeros((10, 13, 4), dtype=torch.int32), torch.zeros((10, 13), dtype=torch.int32), table,
                        20.0, 2, 3)
