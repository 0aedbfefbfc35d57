"""tests/golden/bf16_sites_parent.npz is more than "whatever the parent commit did": for the pass-through multi_cast
case its entries are the round-to-nearest-even of the input's bits wherever IEEE leaves no choice (zeros, normal numbers,
infinities), and NaN where the input is NaN.  fp32 subnormals are left to the fixture (DESIGN.md says what the hardware
did with them).  The premises of the rounding family (tests/bf16_sites_cases.py) are asserted as well, so that an edit
of the family cannot quietly drop the cases the fixture is there for."""
from pathlib import Path

import numpy as np
import pytest

import bf16_sites_cases as cases

FIXTURE = Path(__file__).resolve().parent / "golden" / "bf16_sites_parent.npz"


def rne(u):
    """bf16 bits of fp32 bits, round to nearest, ties to even (not meant for NaN)."""
    u = u.astype(np.uint64)
    return (((u + 0x7FFF + ((u >> 16) & 1)) >> 16) & 0xFFFF).astype(np.uint16)


def classes(u):
    exp, mant = (u >> 23) & 0xFF, u & 0x7FFFFF
    return {"zero": (exp == 0) & (mant == 0), "subnormal": (exp == 0) & (mant != 0), "inf": (exp == 255) & (mant == 0),
            "nan": (exp == 255) & (mant != 0), "normal": (exp > 0) & (exp < 255)}


def test_the_family_holds_what_it_is_there_for():
    u = cases.family_bits()
    kind = classes(u)
    assert u.size == 96 and np.unique(u).size == 96
    assert all(k.any() for k in kind.values())
    tie = kind["normal"] & ((u & 0xFFFF) == 0x8000)
    kept_odd = ((u >> 16) & 1) == 1
    assert (tie & ~kept_odd).any() and (tie & kept_odd).any()                    # a tie that rounds down, one that rounds up
    assert (rne(u[tie & ~kept_odd]) == (u[tie & ~kept_odd] >> 16)).all()
    assert (rne(u[tie & kept_odd]) == (u[tie & kept_odd] >> 16) + 1).all()
    overflow = kind["normal"] & ((rne(u) & 0x7FFF) == 0x7F80)
    assert overflow.any() and ((u[overflow] >> 16) & 0x7FFF == 0x7F7F).all()     # the largest finite value -> infinity
    assert (kind["nan"] & ((u >> 16) & 0x7F == 0)).any()                         # a NaN a truncation would turn into inf
    signs = u >> 31
    assert (signs == 0).sum() == (signs == 1).sum() == 48


@pytest.mark.parametrize("n", cases.LENGTHS)
def test_the_recorded_cast_is_round_to_nearest_even(n):
    with np.load(FIXTURE) as z:
        got = z[f"cast_{n}"]
    u = cases.family(n).numpy().view(np.uint32)
    assert got.dtype == np.uint16 and got.shape == u.shape
    kind = classes(u)
    exact = kind["zero"] | kind["normal"] | kind["inf"]
    assert exact.sum() > n // 2
    assert np.array_equal(got[exact], rne(u[exact]))
    out_is_nan = ((got & 0x7F80) == 0x7F80) & ((got & 0x007F) != 0)
    assert np.array_equal(out_is_nan, kind["nan"])                               # NaN in -> NaN out, and nothing else is NaN
    sub = kind["subnormal"]
    kept = np.array_equal(got[sub], rne(u[sub]))
    flushed = np.array_equal(got[sub], (u[sub] >> 16).astype(np.uint16) & 0x8000)
    print(f"cast_{n}: {int(sub.sum())} subnormal inputs: rounded like normals: {kept}, flushed to signed zero: {flushed}")
