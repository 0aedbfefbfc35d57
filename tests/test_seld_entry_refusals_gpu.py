"""What the seven SELD evaluation entry points of libseld_hip.so refuse, and with which code: one table, called through
the C ABI with raw pointers.  Every case is refused before the launch (or is an empty call), so nothing runs on the device;
the library only has to be initialised for it.  The codes are the ones the entry points returned before their argument
checks were folded into check_decode_args / check_match_args (csrc/seld_eval_core.h, csrc/seld_match_core.h)."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED = -1, -4
DECODE = ("seld_grid_decode", "seld_grid_decode_tta", "seld_grid_decode_refine")
MATCH = ("seld_doa_match", "seld_doa_match_dirs", "seld_doa_match_prefix", "seld_doa_assign")
OUTPUTS = {"seld_grid_decode": ("det_cell", "det_score", "det_count"),
           "seld_grid_decode_tta": ("det_cell", "det_score", "det_count"),
           "seld_grid_decode_refine": ("det_cell", "det_score", "det_count", "det_dir"),
           "seld_doa_match": ("out_a", "out_b"), "seld_doa_match_dirs": ("out_a", "out_b"),
           "seld_doa_match_prefix": ("out_a", "out_b"), "seld_doa_assign": ("out_a",)}


def _cases():
    """(entry point, case, overrides of the good call, expected return code)."""
    rows = []
    for name in DECODE + MATCH:
        outs = OUTPUTS[name]
        rows += [(name, "K = 0", {"K": 0}, INVALID), (name, "K = 9", {"K": 9}, INVALID),
                 (name, "nq = -1", {"nq": -1}, INVALID),
                 # the refined decode asks for det_dir, and the assignment for pair_dist, before it looks at nq
                 (name, "nq = 0, null outputs", dict({o: None for o in outs}, nq=0),
                  INVALID if name in ("seld_grid_decode_refine", "seld_doa_assign") else 0),
                 (name, "nq = 1, null output", {outs[0]: None}, INVALID)]
    for name in DECODE:
        rows += [(name, "W != ceil(total / 50)", {"W": 3}, INVALID), (name, "w0 + nw > W", {"w0": 1}, INVALID),
                 (name, "is_bf16 = 2", {"is_bf16": 2}, INVALID)]
    for name in DECODE[1:]:
        rows += [(name, "pattern 16", {"patterns": (0, 16)}, INVALID),
                 (name, "duplicate pattern", {"patterns": (3, 3)}, INVALID)]
    rows.append(("seld_grid_decode_refine", "n_patterns = 0, patterns not null", {"patterns": (0,), "n_patterns": 0},
                 INVALID))
    for name in MATCH[1:]:
        rows.append((name, "det_dir 4 bytes off", {"det_dir": "offset"}, UNSUPPORTED))
    return rows


CASES = _cases()


def _call(lib, name, buf, stream, overrides):
    """The good call of ``name`` on nq = 1 with ``overrides`` applied; every pointer is the one small device buffer."""
    p = ctypes.c_void_p(buf.data_ptr())
    a = {"logits": p, "is_bf16": 0, "w0": 0, "nw": 2, "W": 2, "total": 100, "first": p, "length": p, "q0": 0, "nq": 1,
         "patterns": (0,) if name == "seld_grid_decode_tta" else (), "threshold": 0.5, "K": 4, "cell_unit": p,
         "det_cell": p, "det_score": p, "det_count": p, "det_dir": p, "probs": None, "ref_offsets": p, "ref_dirs": p,
         "I": 18, "J": 36, "thr_deg": 20.0, "out_a": p, "out_b": p}
    a.update(overrides)
    if a["det_dir"] == "offset":
        a["det_dir"] = ctypes.c_void_p(buf[1:].data_ptr())
    pats = np.asarray(a["patterns"], dtype=np.int32)
    pat_ptr = pats.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)) if len(pats) else None
    n_pat = a.get("n_patterns", len(pats))
    head = (a["logits"], a["is_bf16"], a["w0"], a["nw"], a["W"], a["total"], a["first"], a["length"], a["q0"], a["nq"])
    dets = (a["det_cell"], a["det_score"], a["det_count"])
    refs = (a["det_count"], a["K"], a["ref_offsets"], a["ref_dirs"], a["nq"])
    if name == "seld_grid_decode":
        return lib.seld_grid_decode(*head, a["threshold"], a["K"], *dets, a["probs"], stream)
    if name == "seld_grid_decode_tta":
        return lib.seld_grid_decode_tta(*head, pat_ptr, n_pat, a["threshold"], a["K"], *dets, a["probs"], stream)
    if name == "seld_grid_decode_refine":
        return lib.seld_grid_decode_refine(*head, pat_ptr, n_pat, a["threshold"], a["K"], a["cell_unit"], *dets,
                                           a["det_dir"], a["probs"], stream)
    if name == "seld_doa_match":
        return lib.seld_doa_match(a["det_cell"], *refs, a["I"], a["J"], a["thr_deg"], a["out_a"], a["out_b"], stream)
    if name == "seld_doa_match_dirs":
        return lib.seld_doa_match_dirs(a["det_dir"], *refs, a["thr_deg"], a["out_a"], a["out_b"], stream)
    if name == "seld_doa_match_prefix":
        return lib.seld_doa_match_prefix(a["det_cell"], a["det_dir"], *refs, a["I"], a["J"], a["thr_deg"], a["out_a"],
                                         a["out_b"], stream)
    return lib.seld_doa_assign(a["det_cell"], a["det_dir"], *refs, a["I"], a["J"], a["thr_deg"], a["out_a"], stream)


@pytest.fixture(scope="module")
def library(gpu_device):
    import seld_native
    seld_native.ensure_init(gpu_device)
    buf = torch.full((64,), 77.0, dtype=torch.float32, device=gpu_device)       # 256 bytes, 256-byte aligned
    assert buf.data_ptr() % 16 == 0
    yield seld_native.load_library(), buf, seld_native._stream_ptr(gpu_device)
    torch.cuda.synchronize(gpu_device)
    assert bool((buf == 77.0).all())                                           # nothing was launched on it


@pytest.mark.parametrize("name,case,overrides,expected", CASES, ids=[f"{c[0]}-{c[1]}" for c in CASES])
def test_entry_point_refuses(library, name, case, overrides, expected):
    lib, buf, stream = library
    rc = _call(lib, name, buf, stream, overrides)
    print(name, case, rc, lib.seld_last_error())
    assert rc == expected
    if expected:
        assert lib.seld_last_error().startswith(name.encode() + b":")


def test_the_table_covers_every_entry_point():
    assert {c[0] for c in CASES} == set(DECODE + MATCH) and len(CASES) == 52
