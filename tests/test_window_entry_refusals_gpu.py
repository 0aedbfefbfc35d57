"""What the five window-gather entry points of libseld_hip.so refuse, and with which code: one table, called through the C
ABI with raw pointers.  Every case is refused before the launch (or is an empty call), so nothing runs on the device; the
library only has to be initialised for it.  The codes are the ones the entry points returned before their argument checks
were folded into check_window_args (csrc/augment_core.h).  One fault per case: everything else is the good call."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED = -1, -4
FEATURES = ("seld_window_gather_augment", "seld_window_gather_rotate")
LABELS = ("seld_window_permute_mask", "seld_window_permute_mask_rotate")
ENTRY_POINTS = ("seld_window_gather",) + FEATURES + LABELS
POINTERS = {"seld_window_gather": ("src", "starts", "dst"),
            "seld_window_gather_augment": ("src", "starts", "params", "dst", "table"),
            "seld_window_gather_rotate": ("src", "rot", "starts", "params", "dst", "table"),
            "seld_window_permute_mask": ("src", "starts", "params", "dst"),
            "seld_window_permute_mask_rotate": ("src", "starts", "params", "dst")}
# a window of 2^31 16-byte chunks: 64 chunks per frame at 4 channels, 81 at 18 x 36 cells
TOO_LARGE = {name: (1 << 31) // 64 for name in FEATURES}
TOO_LARGE.update({name: -(-(1 << 31) // 81) for name in LABELS})

GOOD_TABLE = np.tile(np.arange(4, dtype=np.uint8), (16, 1))
BAD_TABLE = GOOD_TABLE.copy()
BAD_TABLE[3, 2] = 4                                          # names a channel that is not there


def _cases():
    """(entry point, case, overrides of the good call, expected return code)."""
    rows = []
    for name in ENTRY_POINTS:
        rows += [(name, "total_rows = -1", {"total_rows": -1}, INVALID), (name, "B = -1", {"B": -1}, INVALID),
                 (name, "window = 0", {"window": 0}, INVALID),
                 (name, "B = 1, null src", {"src": None}, INVALID), (name, "B = 1, null dst", {"dst": None}, INVALID),
                 (name, "B = 0, every pointer null", dict({p: None for p in POINTERS[name]}, B=0), 0)]
    rows.append(("seld_window_gather", "row_bytes = 24", {"row_bytes": 24}, UNSUPPORTED))
    for name in FEATURES + LABELS:
        rows.append((name, "2^31 chunks in a window", {"window": TOO_LARGE[name]}, UNSUPPORTED))
    for name in FEATURES:
        rows += [(name, "channel table names a channel >= channels", {"table": BAD_TABLE}, INVALID),
                 (name, "freq_channels > channels", {"freq_channels": 5}, INVALID),
                 (name, "B = 0, every pointer null, bad channel table",
                  dict({p: None for p in POINTERS[name]}, B=0, table=BAD_TABLE), 0)]
    rows.append(("seld_window_gather_augment", "channels = 65", {"channels": 65}, UNSUPPORTED))
    name = "seld_window_gather_rotate"
    rows += [(name, "channels = 5", {"channels": 5}, UNSUPPORTED), (name, "ch_x == ch_y", {"ch_y": 3}, INVALID),
             (name, "J = 34", {"J": 34}, UNSUPPORTED), (name, "J = 76", {"J": 76}, UNSUPPORTED),
             (name, "B = 1, null rot", {"rot": None}, INVALID), (name, "B = 1, null channel table", {"table": None}, INVALID)]
    for name in LABELS:
        rows += [(name, "I = 0", {"I": 0}, INVALID), (name, "J = 34", {"J": 34}, UNSUPPORTED),
                 (name, "I*J = 20*6", {"I": 20, "J": 6}, UNSUPPORTED),          # a multiple of 8 cells, but J % 4 != 0
                 (name, "I*J = 5*4", {"I": 5, "J": 4}, UNSUPPORTED)]            # J % 4 == 0, but no multiple of 8 cells
    return rows


CASES = _cases()


def _call(lib, name, buf, stream, overrides):
    """The good call of ``name`` on B = 1, window = 1 with ``overrides`` applied; every device pointer is the one small
    buffer (large enough for the good call's one frame, which is never launched)."""
    p = ctypes.c_void_p(buf.data_ptr())
    a = {"src": p, "rot": p, "starts": p, "params": p, "dst": p, "table": GOOD_TABLE, "total_rows": 1, "B": 1, "window": 1,
         "row_bytes": 16, "channels": 4, "freq_channels": 4, "ch_x": 3, "ch_y": 1, "ch_z": 2, "I": 18, "J": 36}
    a.update(overrides)
    table = ctypes.c_void_p(a["table"].ctypes.data) if a["table"] is not None else None
    if name == "seld_window_gather":
        return lib.seld_window_gather(a["src"], a["total_rows"], a["row_bytes"], a["starts"], a["B"], a["window"], a["dst"],
                                      stream)
    if name == "seld_window_gather_augment":
        return lib.seld_window_gather_augment(a["src"], a["total_rows"], a["channels"], a["freq_channels"], a["starts"],
                                              a["params"], a["B"], a["window"], table, 0.0, a["dst"], stream)
    if name == "seld_window_gather_rotate":
        return lib.seld_window_gather_rotate(a["src"], a["rot"], a["total_rows"], a["channels"], a["freq_channels"], a["ch_x"],
                                             a["ch_y"], a["ch_z"], a["J"], a["starts"], a["params"], a["B"], a["window"], table,
                                             0.0, a["dst"], stream)
    return getattr(lib, name)(a["src"], a["total_rows"], a["I"], a["J"], a["starts"], a["params"], a["B"], a["window"],
                              a["dst"], stream)


@pytest.fixture(scope="module")
def library(gpu_device):
    import seld_native
    seld_native.ensure_init(gpu_device)
    buf = torch.full((1024,), 77.0, dtype=torch.float32, device=gpu_device)      # 4 KiB: one frame of any good call
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
    assert {c[0] for c in CASES} == set(ENTRY_POINTS) and len(ENTRY_POINTS) == 5 and len(CASES) == 56
