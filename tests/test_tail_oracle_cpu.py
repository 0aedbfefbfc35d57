"""CPU pins of the float64 oracles of the BatchNorm tails and the depthwise conv (oracle/convtail.py, oracle/dwconv.py)
and of the checks built on them (tests/tail_checks.py):

  * ``fmaf_exact`` is libm's ``fmaf`` bit for bit, ``round_bf16`` is torch's cast;
  * with rounding switched off the oracles equal the stock float64 modules and their autograd;
  * the checks accept an fp32 restatement of the kernels' arithmetic and reject every deliberately wrong variant of it.
"""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import tail_checks as tc
from oracle import convtail as oc
from oracle import dwconv as od

F64 = torch.float64


# ------------------------------------------------------------------------------------------- fmaf / bf16 pins

def _libm_fmaf():
    libm = ctypes.CDLL("libm.so.6")
    libm.fmaf.restype = ctypes.c_float
    libm.fmaf.argtypes = [ctypes.c_float] * 3
    return libm.fmaf


def _same_bits(got, want):
    return np.array_equal(np.asarray(got, dtype=np.float32).view(np.int32), np.asarray(want, dtype=np.float32).view(np.int32))


def test_fmaf_exact_equals_libm_on_random_triples():
    fmaf = _libm_fmaf()
    rng = np.random.default_rng(7)
    n = 120000

    def draw(spread):
        return (rng.standard_normal(n) * np.exp2(rng.integers(-spread, spread + 1, n))).astype(np.float32)

    x, a, b = draw(20), draw(20), draw(40)
    # a third of the addends nearly cancel the product, a third are bf16-valued operands
    b[: n // 3] = -(x[: n // 3].astype(np.float64) * a[: n // 3]).astype(np.float32) * \
        (1 + rng.integers(-3, 4, n // 3) * 2.0 ** -23).astype(np.float32)
    k = 2 * n // 3
    x[k:] = torch.from_numpy(x[k:]).bfloat16().float().numpy()
    got = oc.fmaf_exact(*(torch.from_numpy(v).double() for v in (x, a, b))).numpy()
    want = np.array([fmaf(float(p), float(q), float(r)) for p, q, r in zip(x, a, b)], dtype=np.float32)
    assert np.isfinite(want).all()
    assert _same_bits(got, want)
    # and it is not the double-rounded product-then-add
    naive = (x.astype(np.float64) * a).astype(np.float32) + b
    assert not _same_bits(naive, want)


def test_fmaf_exact_equals_libm_on_constructed_cases():
    fmaf = _libm_fmaf()
    e = 2.0 ** -23
    cases = [
        # product 1 - 2^-46; sum = the midpoint 2^24 + 3 minus a remainder float64 cannot hold: down, not to even
        (1 + e, 1 - e, 2.0 ** 24 + 2, 2.0 ** 24 + 2),
        # product -(1 - 2^-46); sum = the midpoint 2^24 + 1 plus that remainder: up, away from even
        (-(1 + e), 1 - e, 2.0 ** 24 + 2, 2.0 ** 24 + 2),
        (-(1 + e), 1 - e, 2.0 ** 24 + 4, 2.0 ** 24 + 4),
        # exact ties: to even
        (1.0, 1.0, 2.0 ** 24 + 2, 2.0 ** 24 + 4),
        (-1.0, 1.0, 2.0 ** 24 + 2, 2.0 ** 24),
        # cancellation to a subnormal: 2^-126 (2^-22 + 2^-46) -> 2^-148
        (2.0 ** -63 * (1 + e), 2.0 ** -63 * (1 + e), -(2.0 ** -126), 2.0 ** -148),
        # ... and to below half the smallest subnormal
        (2.0 ** -63 * (1 + e), 2.0 ** -63 * (1 + e), -(2.0 ** -126) * (1 + 2 * e), 0.0),
        # subnormal midpoints with a remainder: 1.5 * 2^-149 - tiny -> 2^-149;  0.5 * 2^-149 - tiny -> 0
        (2.0 ** -75 * (1 + e), 2.0 ** -75 * (1 - e), 2.0 ** -149, 2.0 ** -149),
        (2.0 ** -75 * (1 + e), 2.0 ** -75 * (1 - e), 0.0, 0.0),
        (-(2.0 ** -75) * (1 + e), 2.0 ** -75 * (1 - e), 2.0 ** -148, 2.0 ** -148),
    ]
    for x, a, b, expect in cases:
        for v in (x, a, b):
            assert float(np.float32(v)) == v                    # the case is what it says: fp32 operands
        want = fmaf(x, a, b)
        got = float(oc.fmaf_exact(torch.tensor([x], dtype=F64), torch.tensor([a], dtype=F64),
                                  torch.tensor([b], dtype=F64))[0])
        assert want == expect, (x, a, b, want, expect)
        assert _same_bits([got], [want]), (x, a, b, got, want)


def test_add_exact_is_the_fp32_add():
    rng = np.random.default_rng(8)
    n = 50000
    u = (rng.standard_normal(n) * np.exp2(rng.integers(-30, 31, n))).astype(np.float32)
    v = (rng.standard_normal(n) * np.exp2(rng.integers(-30, 31, n))).astype(np.float32)
    got = oc.add_exact(torch.from_numpy(u).double(), torch.from_numpy(v).double()).numpy()
    assert _same_bits(got, u + v)


def test_round_bf16_equals_torch_cast():
    g = torch.Generator().manual_seed(9)
    v = torch.randn(200000, generator=g) * torch.exp2(torch.randint(-40, 40, (200000,), generator=g).float())
    ties = (torch.arange(-4096, 4096, dtype=torch.int32) * 0x8000 + 0x3F800000).view(torch.float32)   # every half-way case
    v = torch.cat([v, ties, -ties, torch.tensor([0.0, -0.0, 3.0e38, -3.0e38, 1e-40])])
    want = v.bfloat16()
    for src in (v, v.double()):
        got = oc.round_bf16(src)
        assert got.dtype == src.dtype
        assert torch.equal(got.float().view(torch.int32), want.float().view(torch.int32))


# ------------------------------------------------------------------------------------------- stock-module pins

def _close(got, want, name):
    err = (got - want).abs().max().item()
    assert err <= 1e-12 * (want.abs().max().item() + 1e-30), (name, err)


def _rows(t):
    """[B, C, T, F] -> [rows, C] in channels-last row order."""
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


@pytest.mark.parametrize("mode", [1, 2, 3, 4])
@pytest.mark.parametrize("shape", [(2, 8, 3, 4), (3, 16, 5, 6)])
def test_unrounded_oracle_equals_stock_float64_modules(mode, shape):
    g = torch.Generator().manual_seed(100 * mode + shape[1])
    b, c, t, f = shape
    x = (torch.randn(shape, generator=g, dtype=F64) * 1.5 + 0.3).requires_grad_(True)
    res = torch.randn(shape, generator=g, dtype=F64).requires_grad_(True) if mode == 3 else None
    bn = (nn.BatchNorm1d(c) if mode == 4 else nn.BatchNorm2d(c)).double()
    with torch.no_grad():
        bn.weight.copy_(torch.rand(c, generator=g, dtype=F64) + 0.5)
        bn.bias.copy_(torch.randn(c, generator=g, dtype=F64) * 0.3)
        bn.running_mean.copy_(torch.randn(c, generator=g, dtype=F64))
        bn.running_var.copy_(torch.rand(c, generator=g, dtype=F64) + 0.5)
    rm0, rv0 = bn.running_mean.clone(), bn.running_var.clone()
    if mode == 1:
        y = torch.relu(bn(x))
    elif mode == 2:
        y = nn.MaxPool2d((1, 2))(torch.relu(bn(x)))
    elif mode == 3:
        y = torch.relu(bn(x) + res)
    else:
        xm = _rows(x.detach()).clone().requires_grad_(True)
        y = F.silu(bn(xm))
    dy = torch.randn(y.shape, generator=g, dtype=F64)
    y.backward(dy)

    x2 = _rows(x.detach())
    r2 = None if res is None else _rows(res.detach())
    y2, dy2 = (y.detach(), dy) if mode == 4 else (_rows(y.detach()), _rows(dy))
    st = oc.tail_stats(x2, bn.weight.detach(), bn.bias.detach(), bn.eps, rm0, rv0, bn.momentum, True)
    _close(st["running_mean"], bn.running_mean, "running_mean")
    _close(st["running_var"], bn.running_var, "running_var")
    fwd = oc.tail_forward_replay(x2, r2, st["a"], st["b"], mode, F64)
    _close(fwd["y"], y2, "y")
    sums = oc.tail_backward_replay(x2, dy2, fwd, mode, st["mean"], st["invstd"])
    _close(sums["sum_dz"], bn.bias.grad, "dbias")
    _close(sums["sum_dzx"], bn.weight.grad, "dweight")
    rep = oc.tail_backward_replay(x2, dy2, fwd, mode, st["mean"], st["invstd"], sums["sum_dzx"], sums["sum_dz"], st["a"])
    _close(rep["dx"], xm.grad if mode == 4 else _rows(x.grad), "dx")
    if mode == 3:
        _close(rep["dres"], _rows(res.grad), "dres")
    # eval mode: coefficients from the running statistics, which stay
    bn.eval()
    rm1, rv1 = bn.running_mean.clone(), bn.running_var.clone()
    ev = oc.tail_stats(x2, bn.weight.detach(), bn.bias.detach(), bn.eps, rm1, rv1, bn.momentum, False)
    z_ref = bn(x2 if mode == 4 else x.detach())
    _close(x2 * ev["a"] + ev["b"], z_ref.detach() if mode == 4 else _rows(z_ref.detach()), "eval z")
    assert torch.equal(ev["running_mean"], rm1) and torch.equal(ev["running_var"], rv1)


@pytest.mark.parametrize("b,t,d,k", [(2, 9, 8, 5), (3, 40, 16, 31), (1, 4, 8, 31), (2, 7, 8, 1)])
def test_dwconv_oracle_equals_stock_float64_conv1d(b, t, d, k):
    g = torch.Generator().manual_seed(b * 100 + t)
    x = torch.randn(b, t, d, generator=g, dtype=F64, requires_grad=True)
    w = torch.randn(d, 1, k, generator=g, dtype=F64, requires_grad=True)
    bias = torch.randn(d, generator=g, dtype=F64, requires_grad=True)
    y = F.conv1d(x.transpose(1, 2), w, bias, padding=(k - 1) // 2, groups=d).transpose(1, 2)
    dy = torch.randn(y.shape, generator=g, dtype=F64)
    y.backward(dy)
    w2 = w.detach().reshape(d, k)
    got, mag = od.forward(x.detach(), w2, bias.detach())
    _close(got, y.detach(), "y")
    assert (mag >= got.abs() * (1 - 1e-12)).all()
    _close(od.forward(x.detach(), w2, None)[0], y.detach() - bias.detach(), "y without bias")
    _close(od.dgrad(dy, w2)[0], x.grad, "dx")
    dw, dw_mag, db, db_mag = od.wgrad(x.detach(), dy, k)
    _close(dw, w.grad.reshape(d, k), "dweight")
    _close(db, bias.grad, "dbias")
    assert (dw_mag >= dw.abs() * (1 - 1e-12)).all() and (db_mag >= db.abs() * (1 - 1e-12)).all()


# ------------------------------------------------------------------------------------------- emulation and mutants

def _f32(v):
    return v.to(torch.float32)


def emulate_tail(x, res, dy, weight, bias, eps, momentum, rm0, rv0, mode, mutant=None):
    """The kernels' arithmetic restated on the CPU: statistics combined in double from (here: exact) sums and stored as
    fp32, the element-wise stages as fp32 fused multiply-adds (``fmaf_exact``) with the activation dtype's rounding.
    ``mutant`` names one deliberate defect.  -> dict of the kernels' outputs in their dtypes."""
    dtype = x.dtype
    rnd = oc.round_bf16 if dtype == torch.bfloat16 else (lambda v: v)
    x64, dy64 = x.to(F64), dy.to(F64)
    rows = x64.shape[0]
    kept = x64[:-1] if mutant == "row_dropped" else x64
    st = oc.tail_stats(kept, weight, bias, tc.c_float(eps), rm0, rv0, tc.c_float(momentum), True)
    mean, invstd = _f32(st["mean"]), _f32(st["invstd"])
    a = _f32(weight.to(F64) * st["invstd"])                                      # one rounding, from the double invstd
    b = _f32(oc.fmaf_exact(-mean.to(F64), a.to(F64), bias.to(F64)))
    a64, b64, mean64, invstd64 = a.to(F64), b.to(F64), mean.to(F64), invstd.to(F64)

    relu = lambda v: torch.where(v > 0, v, torch.zeros((), dtype=F64))
    xin = torch.roll(x64, -1, 0) if mutant == "pair_shift" else x64             # pairs (2o + 1, 2o + 2)
    zu = oc.fmaf_exact(xin, a64, b64)
    z = rnd(zu)
    zc = zu if mutant == "unrounded" else z                                      # what the comparisons see
    dsilu = None
    if mode == 1:
        y, route = rnd(relu(zc)), torch.where(zc > 0, 0, -1)
    elif mode == 2:
        r0, r1 = relu(zc[0::2]), relu(zc[1::2])
        second = r1 >= r0 if mutant == "tie_second" else r1 > r0
        m = torch.where(second, r1, r0)
        y, route = rnd(m), torch.where(m > 0, second.long(), -1)
    elif mode == 3:
        if mutant == "res_after_relu":
            y, route = rnd(oc.add_exact(relu(z), res.to(F64))), torch.where(z > 0, 0, -1)
        else:
            t = rnd(oc.add_exact(zc, res.to(F64)))
            y, route = relu(t), torch.where(t > 0, 0, -1)
    else:
        y, dsilu = rnd(_f32(oc.silu(z)).to(F64)), _f32(oc.silu_grad(z)).to(F64)

    if mode == 4:
        dz = _f32(dy64 * dsilu).to(F64)
    elif mode == 2:
        dz = torch.zeros_like(x64)
        dz[0::2] = torch.where(route == 0, dy64, 0.0)
        dz[1::2] = torch.where(route == 1, dy64, 0.0)
        if mutant == "pair_shift":
            dz = torch.roll(dz, 1, 0)
    else:
        dz = torch.where(route == 0, dy64, 0.0)
    cut = slice(0, rows - 1) if mutant == "row_dropped" else slice(None)
    s_dz = dz[cut].sum(0)
    s_dzx = (dz * _f32(x64 - mean64).to(F64))[cut].sum(0) * invstd64
    q64 = -a64 * (s_dzx / rows) * invstd64
    p = _f32(-a64 * (s_dz / rows) - q64 * mean64).to(F64)
    q = _f32(q64).to(F64)
    dx = rnd(oc.fmaf_exact(a64, dz, oc.fmaf_exact(q, x64, p)))
    y, dx = y.to(dtype), dx.to(dtype)
    if mutant == "last_row_unwritten":
        y[-1], dx[-1] = 1.0, 1.0
    out = dict(y=y, mean_invstd=torch.stack([mean, invstd]), scale_shift=torch.stack([a, b]),
               running_mean=_f32(st["running_mean"]), running_var=_f32(st["running_var"]),
               dx=dx, dweight=_f32(s_dzx), dbias=_f32(s_dz), dres=dz.to(dtype) if mode == 3 else None)
    if mutant and mutant.startswith("nan_"):                                     # one NaN in one output
        target = out[mutant[4:]]
        target[(1, 3) if target.dim() == 2 and target.shape[0] > 2 else 1] = float("nan")
    return out


def _emulate(case, mode, mutant=None):
    return emulate_tail(case["x"], case["res"], case["dy"], case["weight"], case["bias"], 1e-5, 0.1, case["rm0"],
                        case["rv0"], mode, mutant)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("mode", [1, 2, 3, 4])
@pytest.mark.parametrize("integer", [True, False])
def test_checks_accept_the_unmutated_emulation(mode, dtype, integer):
    case = tc.make_case(mode, dtype, integer=integer)
    ratios = tc.run_checks(case, _emulate(case, mode), mode, exact_stats=integer)
    assert tc.passes(ratios), tc.fmt(ratios)


# (mutant, mode, the checks that must reject it, wide_bias)
MUTANTS = [
    ("tie_second", 2, ["backward.dx"], False),
    ("unrounded", 2, ["backward.dx"], True),
    ("unrounded", 3, ["forward.y"], False),
    ("pair_shift", 2, ["forward.y", "backward.dx"], False),
    ("row_dropped", 1, ["stats.mean", "backward.dbias"], False),
    ("row_dropped", 4, ["stats.mean", "backward.dbias", "backward.dweight"], False),
    ("last_row_unwritten", 1, ["forward.y", "backward.dx"], False),
    ("last_row_unwritten", 2, ["forward.y", "backward.dx"], False),
    ("last_row_unwritten", 4, ["forward.y", "backward.dx"], False),
    ("res_after_relu", 3, ["forward.y"], False),
    # a single NaN: in an output, in a parameter gradient (which also makes the dx reference a NaN), in a coefficient
    # (from which the replay would reproduce the NaN bit for bit)
    ("nan_dx", 1, ["backward.dx"], False),
    ("nan_dx", 2, ["backward.dx"], False),
    ("nan_dx", 4, ["backward.dx"], False),
    ("nan_dweight", 1, ["backward.dweight", "backward.dx"], False),
    ("nan_dweight", 4, ["backward.dweight", "backward.dx"], False),
    ("nan_dbias", 4, ["backward.dbias", "backward.dx"], False),
    ("nan_y", 4, ["forward.y"], False),
    ("nan_y", 2, ["forward.y"], False),
    ("nan_dres", 3, ["backward.dres"], False),
    ("nan_scale_shift", 1, ["stats.finite", "forward.y", "backward.dx"], False),
    ("nan_mean_invstd", 4, ["stats.finite", "backward.dx"], False),
    ("nan_running_var", 1, ["stats.finite"], False),
]


@pytest.mark.parametrize("mutant,mode,rejected_by,wide_bias", MUTANTS)
def test_checks_reject_every_mutant(mutant, mode, rejected_by, wide_bias):
    case = tc.make_case(mode, torch.bfloat16, rows=512 if wide_bias else 74, integer=not wide_bias, seed=3,
                      wide_bias=wide_bias)
    good = tc.run_checks(case, _emulate(case, mode), mode, exact_stats=not wide_bias)
    assert tc.passes(good), tc.fmt(good)
    bad = tc.run_checks(case, _emulate(case, mode, mutant), mode, exact_stats=not wide_bias)
    for name in rejected_by:
        assert not bad[name] <= 1.0, (mutant, name, tc.fmt(bad))
    assert not tc.passes(bad) and tc.worst(bad) > 1.0, (mutant, tc.fmt(bad))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("mode", [1, 2, 3, 4])
def test_a_nan_in_any_output_fails_the_pass_criterion(mode, dtype):
    """Whatever the position of its ratio among the others: a NaN in any single output must fail ``passes``."""
    case = tc.make_case(mode, dtype, integer=mode != 4, seed=11)
    outputs = ["y", "dx", "dweight", "dbias", "mean_invstd", "scale_shift", "running_mean", "running_var"]
    for name in outputs + (["dres"] if mode == 3 else []):
        bad = tc.run_checks(case, _emulate(case, mode, "nan_" + name), mode, exact_stats=mode != 4)
        assert not tc.passes(bad) and tc.worst(bad) == float("inf"), (name, tc.fmt(bad))


def test_pass_criterion_sees_a_nan_ratio_in_any_position():
    nan = float("nan")
    for ratios in ({"a": nan, "b": 0.5}, {"a": 0.5, "b": nan}, {"a": 0.2, "b": nan, "c": 0.9}):
        assert not tc.passes(ratios) and tc.worst(ratios) == float("inf")
    assert tc.passes({"a": 0.5, "b": 1.0}) and tc.worst({"a": 0.5, "b": 1.0}) == 1.0
    assert not tc.passes({"a": 0.5, "b": float("inf")})
    one = torch.ones(3, dtype=F64)
    assert tc.ratio(torch.tensor([0.0, nan, 0.0], dtype=F64), one) == float("inf")
    assert tc.ratio(one, torch.tensor([1.0, nan, 1.0], dtype=F64)) == float("inf")
    assert tc.mismatch(torch.tensor([nan, 1.0]), torch.tensor([nan, 1.0], dtype=F64)) == float("inf")


def _dw_case(dtype, b=2, t=101, d=8, k=31, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(b, t, d, generator=g).to(dtype)
    dy = torch.randn(b, t, d, generator=g).to(dtype)
    return x, dy, torch.randn(d, k, generator=g) * 0.2, torch.randn(d, generator=g)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_dwconv_checks_accept_the_rounded_oracle_and_reject_the_mutants(dtype):
    x, dy, w, bias = _dw_case(dtype)
    b, t, d = x.shape
    k = w.shape[1]
    y, y_mag = od.forward(x, w, bias)
    dx, dx_mag = od.dgrad(dy, w)
    dw, dw_mag, db, db_mag = od.wgrad(x, dy, k)
    assert tc.dw_output_ratio(y.to(dtype), y, y_mag, k) <= 1.0
    assert tc.dw_output_ratio(dx.to(dtype), dx, dx_mag, k) <= 1.0
    assert tc.dw_grad_ratio(_f32(dw), dw, dw_mag, b, t) <= 1.0 and tc.dw_grad_ratio(_f32(db), db, db_mag, b, t) <= 1.0
    # a NaN in an output or a gradient
    holed, dw_holed = y.to(dtype).clone(), _f32(dw).clone()
    holed[1, 3, 2], dw_holed[2, 5] = float("nan"), float("nan")
    assert not tc.dw_output_ratio(holed, y, y_mag, k) <= 1.0 and not tc.dw_grad_ratio(dw_holed, dw, dw_mag, b, t) <= 1.0
    assert not tc.passes({"y": 0.5, "dx": tc.dw_output_ratio(holed, y, y_mag, k), "dweight": 0.1})
    # taps not flipped in the data gradient
    assert tc.dw_output_ratio(od.forward(dy, w, None)[0].to(dtype), dx, dx_mag, k) > 1.0
    # a tap read across the batch boundary: the two batch rows convolved as one sequence
    crossed = od.forward(x.reshape(1, b * t, d), w, bias)[0].reshape(b, t, d)
    assert tc.dw_output_ratio(crossed.to(dtype), y, y_mag, k) > 1.0
    # the last time step of a 50-step chunk dropped from the weight gradient
    cut = dy.clone()
    cut[:, 49] = 0
    dw_cut, _, db_cut, _ = od.wgrad(x, cut, k)
    assert tc.dw_grad_ratio(_f32(dw_cut), dw, dw_mag, b, t) > 1.0
    assert tc.dw_grad_ratio(_f32(db_cut), db, db_mag, b, t) > 1.0
