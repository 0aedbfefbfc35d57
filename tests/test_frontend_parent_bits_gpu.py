"""GPU check that the front end -- the log-mel, spectrum / phasor export, STFT and fused FOA kernels of csrc/logmel.hip,
whose per-iteration wave pipeline, workgroup prologue and launch prologue became shared functions, and the GCC-PHAT and
NIPD kernels behind ``spatial_features`` -- still writes every bit the build of the commit before that change wrote for
the same seeded clips: tests/golden/frontend_parent.npz, recorded by tools/record_frontend_parent_golden.py on that
build.  The clips, their zero channel and zero blocks and the families are in tests/frontend_parent_cases.py; results
above 64 KB are compared through their SHA-256."""
import functools
from pathlib import Path

import numpy as np
import pytest
import torch

import frontend_parent_cases as cases

pytestmark = pytest.mark.gpu

FIXTURE = Path(__file__).resolve().parent / "golden" / "frontend_parent.npz"
NAMES = ("logmel_cft", "logmel_tcf", "logmel_strided", "phasors_logmel", "phasors_words", "spectrum_logmel", "spectrum_spec",
         "stft", "logmel_iv", "logmel_gcc_c3", "logmel_gcc_c7", "logmel_nipd_c3")


@functools.lru_cache(maxsize=None)
def fixture():
    return dict(np.load(FIXTURE))


def as_tensor(words):
    return torch.from_numpy(np.ascontiguousarray(words).view(np.int32))


@pytest.mark.parametrize("dtype", cases.DTYPES, ids=("f32", "i16"))
@pytest.mark.parametrize("length", cases.LENGTHS)
def test_front_end_has_the_parent_bits(gpu_device, length, dtype):
    import seld_native
    got = cases.run(seld_native, gpu_device, length, dtype)
    want = fixture()
    assert tuple(got) == NAMES
    for name, x in got.items():
        assert torch.isfinite(x).all() if x.dtype == torch.float32 else True, name
        mine, theirs = cases.record(name, x), want[cases.key(length, dtype, name)]
        assert mine.shape == theirs.shape and torch.equal(as_tensor(mine), as_tensor(theirs)), cases.key(length, dtype, name)
    for name in cases.SAME_LOGMEL:
        assert torch.equal(got[name][:, :, :3], got["phasors_logmel"]), name


def test_fixture_holds_every_case_and_the_strided_placement_keeps_its_surroundings():
    want = fixture()
    assert sorted(want) == sorted(cases.key(length, dtype, name) for length in cases.LENGTHS for dtype in cases.DTYPES
                                  for name in NAMES)
    fill = np.float32(cases.FILL).view(np.uint32)
    for length in cases.LENGTHS:
        for dtype in cases.DTYPES:
            wide = want[cases.key(length, dtype, "logmel_strided")]
            assert (wide[:, :, 0] == fill).all() and (wide[:, :, 4] == fill).all() and (wide[:, :, 1:4] != fill).all()
