"""Every bf16 store that goes through csrc/seld_bf16.h and that no other test compares bit for bit, against what the
commit before that header stored for the same inputs: tests/golden/bf16_sites_parent.npz, recorded on that commit's
library by tools/record_bf16_sites_golden.py (uint16 bit patterns).  The cases, and the list of the sites other tests
already pin, are in tests/bf16_sites_cases.py; tests/test_bf16_sites_cpu.py ties the fixture to round-to-nearest-even."""
import functools
from pathlib import Path

import numpy as np
import pytest

import bf16_sites_cases as cases

pytestmark = pytest.mark.gpu
FIXTURE = Path(__file__).resolve().parent / "golden" / "bf16_sites_parent.npz"
NAMES = ([f"{site}_{n}" for site in ("cast", "adam", "adam_guarded") for n in cases.LENGTHS] +
         ["sum_chunks", "column_sums", "fold_bias", "softmax_mse_grad", "softmax_ce_grad", "smr_loss_grad",
          "conv3x3_wgrad_dw", "prepare_gi_bias", "prepare_w_t", "dwhh_finish"])


@functools.lru_cache(maxsize=None)
def golden():
    with np.load(FIXTURE) as z:
        return {k: z[k] for k in z.files}


_results = {}


def results(device):
    """All cases, run once and left unchanged."""
    import seld_native as nat
    if not _results:
        _results.update({name: cases.bits(t) for name, t in cases.run(nat, device).items()})
    return _results


def test_the_cases_and_the_fixture_name_the_same_sites(gpu_device):
    assert sorted(results(gpu_device)) == sorted(NAMES) == sorted(golden())


@pytest.mark.parametrize("name", NAMES)
def test_stored_bits_equal_the_parent_commits(gpu_device, name):
    got, want = results(gpu_device)[name], golden()[name]
    assert got.dtype == np.uint16 and got.shape == want.shape
    differ = np.flatnonzero(got != want)
    assert differ.size == 0, (name, differ[:8], got[differ[:8]], want[differ[:8]])
    assert np.unique(got).size > 8                                  # something was stored
