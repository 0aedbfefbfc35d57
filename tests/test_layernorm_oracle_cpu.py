"""CPU pins of the float64 LayerNorm oracle (oracle/layernorm.py) and of the checks built on it
(tests/layernorm_checks.py):

  * with rounding switched off the oracle equals float64 ``F.layer_norm`` [+ relu] and its autograd;
  * the input families have the properties the parity tests rely on;
  * the checks accept an fp32 emulation of the kernels (the replay, plus an fp32 dx in two groupings) and reject every
    deliberately wrong variant of it;
  * the wrappers refuse arguments the kernels cannot take, before anything touches a device.
"""
import pytest
import torch
import torch.nn.functional as F

import layernorm_checks as lc
from oracle import layernorm as ol
from oracle.convtail import add_exact, fmaf_exact

F64 = torch.float64
F32, BF16 = torch.float32, torch.bfloat16
WIDTHS = [256, 512, 1024, 2048]


# ------------------------------------------------------------------------------------------- the oracle is LayerNorm

@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("d", WIDTHS)
def test_plain_oracle_is_float64_layer_norm_and_autograd(d, relu):
    g = torch.Generator().manual_seed(d)
    rows, eps = 7, 1e-5
    x = (torch.randn(rows, d, generator=g, dtype=F64) * 3 + 1.5).requires_grad_(True)
    w = (torch.randn(d, generator=g, dtype=F64) * 0.5 + 1).requires_grad_(True)
    b = (torch.randn(d, generator=g, dtype=F64) * 0.2).requires_grad_(True)
    dy = torch.randn(rows, d, generator=g, dtype=F64)
    y = F.layer_norm(x, (d,), w, b, eps)
    if relu:
        y = torch.relu(y)
    y.backward(dy)
    got = ol.plain(x.detach(), w.detach(), b.detach(), eps, relu, dy)
    for name, want in (("y", y.detach()), ("dx", x.grad), ("dweight", w.grad), ("dbias", b.grad)):
        err = (got[name] - want).abs().max().item()
        assert err <= 1e-12 * (want.abs().max().item() + 1e-30), (name, err)
    # the replay functions with every rounding off are the same function
    fwd = ol.forward_replay(x.detach(), w.detach(), b.detach(), got["mean"], got["rstd"], relu, F64)
    assert (fwd["y"] - y.detach()).abs().max().item() <= 1e-12 * y.detach().abs().max().item()


def test_replay_geometry_is_the_dispatch_table():
    for d, (v, k) in ol.GEOMETRY.items():
        assert 64 * v * k == d and ol.sum_depth(d) == d // 64 + 6
        t = torch.arange(d, dtype=F64).view(1, d)
        assert float(ol.lanes(t, d)[0, k - 1, 5, 2]) == ((k - 1) * 64 + 5) * v + 2
    assert [ol.backward_blocks(r) for r in (1, 4, 5, 2045, 2048, 2049, 10 ** 6)] == [1, 1, 2, 512, 512, 512, 512]
    assert ol.column_depth(2048) == 1 + 24 and ol.column_depth(2049) == 2 + 24


# ------------------------------------------------------------------------------------------- premises of the families

@pytest.mark.parametrize("d", WIDTHS)
def test_constant_rows_replay_to_the_constant(d):
    case = lc.make_case("constant", BF16, 9, d)
    mean, ve = ol.row_stats_replay(case["x"].to(F64), 1e-5, d)
    assert torch.equal(mean, case["x"][:, 0].to(F64))
    assert torch.equal(ve, torch.full_like(ve, ol.c_float(1e-5)))
    assert case["x"].float().unique().numel() > 1


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
def test_near_constant_rows_have_variance_about_eps(dtype):
    case = lc.make_case("near_constant", dtype, 65, 256)
    var = case["x"].to(F64).var(1, unbiased=False)
    assert 0.25e-5 <= var.min().item() and var.max().item() <= 4e-5
    assert var.min().item() < 1e-5 < var.max().item()


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("rows,d", [(5, 256), (65, 2048), (2049, 512)])
def test_near_zero_family_sits_on_the_relu_edge(rows, d, dtype):
    case = lc.make_case("near_zero", dtype, rows, d)
    x = case["x"].to(F64)
    mean, rstd = lc.replay_rstd(x, 1e-5)
    fwd = ol.forward_replay(x, case["weight"], case["bias"], mean, rstd, True, dtype)
    z, prod = fwd["z"], fwd["xhat"] * case["weight"].to(F64)
    near = z.abs() <= 2 * lc.ulp32(prod)
    live = case["weight"] != 0
    assert near[:, live].double().mean().item() >= 0.01 and near.double().mean().item() >= 0.01
    assert bool((z[near] > 0).any()) and bool((z[near] < 0).any())
    zero = z == 0
    assert bool((zero & ~torch.signbit(z)).any()) and bool((zero & torch.signbit(z)).any())
    # and the float64 pre-activation takes the other side often enough for the mask mutant to matter
    z64 = ol.plain(x, case["weight"], case["bias"], 1e-5, True)["z"]
    assert int(((z64 > 0) != (z > 0)).sum()) >= 0.001 * z.numel()


def _one_pass_var(x, d):
    """E[x^2] - mean^2 in fp32, accumulated in the kernel's order."""
    v, k = ol.geometry(d)
    xl = ol.lanes(x, d)
    q = torch.zeros(x.shape[0], 64, dtype=F64)
    for c in range(k):
        for j in range(v):
            q = fmaf_exact(xl[:, c, :, j], xl[:, c, :, j], q)
    mean = ol.row_mean_replay(x, d)
    return add_exact(ol.round_f32(ol.wave_sum(q) / d), -ol.round_f32(mean * mean))


def test_offset_family_defeats_the_one_pass_variance():
    """fp32 (mean 4096, std 0.01 .. 1): wrong by more than 100 % on the worst row.  The bf16 family (mean 64, std 1,
    the largest offset whose neighbours bf16 still separates) moves it by about 1e-4 relative only: thousands of ulps
    of rstd, which the bit-sharp rstd check sees, but no 100 %."""
    case = lc.make_case("offset", F32, 65, 256)
    x = case["x"].to(F64)
    var = x.var(1, unbiased=False)
    assert (((_one_pass_var(x, 256) - var).abs() / var).max().item()) > 1.0
    two_pass = ol.row_var_replay(x, ol.row_mean_replay(x, 256), 256)
    assert ((two_pass - var).abs() / var).max().item() < 1e-3


# ------------------------------------------------------------------------------------------- emulation and mutants

def _mul(a, b):
    return ol.round_f32(a * b)                       # the product of two fp32 values is exact in float64


def _lane_chain(terms_of, d, fused):
    """Row sums of kChunks * V terms per lane in (c, j) order + butterfly.  ``terms_of(c, j)`` -> (a, b): the term is
    a * b, accumulated as fmaf(a, b, s) when ``fused`` else s + fp32(a * b)."""
    v, k = ol.geometry(d)
    s = None
    for c in range(k):
        for j in range(v):
            a, b = terms_of(c, j)
            s = torch.zeros_like(a) if s is None else s
            s = fmaf_exact(a, b, s) if fused else add_exact(s, _mul(a, b))
    return ol.wave_sum(s)


def _truncate_bf16(v):
    bits = v.to(torch.float32).contiguous().view(torch.int32) & -65536
    return bits.view(torch.float32).to(F64)


def emulate(case, relu, mutant=None, grouping=0):
    """The kernels in emulated fp32 (float64 tensors holding fp32 values), with one deliberate defect if ``mutant``.
    grouping 0: every product rounded on its own; 1: products contracted into FMAs wherever a compiler may."""
    dtype = case["x"].dtype
    x, dy, w, b = (case[k].to(F64) for k in ("x", "dy", "weight", "bias"))
    rows, d = x.shape
    v, k = ol.geometry(d)
    eps = ol.c_float(case["eps"])
    one = torch.ones((), dtype=F64)
    # ---- statistics
    if mutant == "mean_first_chunk":
        xl = ol.lanes(x, d)
        s = torch.zeros(rows, 64, dtype=F64)
        for j in range(v):
            s = add_exact(s, xl[:, 0, :, j])
        mean = ol.round_f32(ol.wave_sum(s) / (64 * v))
    else:
        mean = ol.row_mean_replay(x, d)
    var = ol.row_var_replay(x, mean, d)
    if mutant == "one_pass_variance":
        var = _one_pass_var(x, d).clamp_min(0.0)
    if mutant == "divisor_d_minus_1":
        var = ol.round_f32(var * d / (d - 1))
    ve = var if mutant == "eps_dropped" else add_exact(var, torch.tensor(eps, dtype=F64))
    rstd = ol.round_f32(1.0 / torch.sqrt(ve))
    if mutant == "eps_after_sqrt":
        rstd = ol.round_f32(1.0 / (torch.sqrt(var) + eps))
    # ---- forward
    w_used, b_used = w, b
    if mutant == "weight_bias_v8_map" and d == 256:
        col = torch.arange(d)
        idx = ((col // 4) * 8 + col % 4) % d
        w_used, b_used = w[idx], b[idx]
    fwd = ol.forward_replay(x, w_used, b_used, mean, rstd, relu, dtype)
    y, z, xh = fwd["y"], fwd["z"], fwd["xhat"]
    if mutant == "bf16_store_truncates" and dtype == BF16:
        y = _truncate_bf16(torch.where(z > 0, z, 0 * one) if relu else z)
    if mutant == "bf16_halves_swapped" and dtype == BF16:
        y = y.view(rows, d // 2, 2).flip(2).reshape(rows, d)
    if mutant == "y_lanes_permuted":
        y = ol.lanes(y, d)[:, :, torch.arange(64) ^ 1, :].reshape(rows, d)
    stats = torch.stack([mean, ve if mutant == "rstd_stored_as_variance" else rstd], 1).float()
    # ---- backward
    zb = fmaf_exact(xh, w, b)
    mask = zb > 0
    if mutant == "mask_z_ge_0":
        mask = zb >= 0
    if mutant == "mask_from_float64_z":
        mask = ol.plain(x, w, b, eps, True)["z"] > 0
    g = torch.where(mask, dy, 0 * one) if relu else dy
    nw = ol.WAVES * ol.backward_blocks(rows)
    seen = slice(0, nw) if mutant == "rows_past_2048_skipped" else slice(None)
    dw_w, db_w = ol.wave_sums(g[seen], xh[seen], nw)
    if mutant == "wave_left_out_of_fold":
        dw_w.view(-1, ol.WAVES, d)[:, ol.WAVES - 1] = 0
        db_w.view(-1, ol.WAVES, d)[:, ol.WAVES - 1] = 0
    pw, pb = ol.block_fold(dw_w), ol.block_fold(db_w)
    if mutant == "last_partial_row_left_out":
        dweight, dbias = ol.final_sum(pw[:-1]), ol.final_sum(pb[:-1])
    else:
        dweight, dbias = ol.final_sum(pw), ol.final_sum(pb)
    if mutant == "partial_row_counted_twice":
        dweight, dbias = add_exact(dweight, pw[-1]), add_exact(dbias, pb[-1])
    if mutant == "dweight_dbias_swapped":
        dweight, dbias = dbias, dweight
    # ---- dx in fp32
    gl, wl, xl = ol.lanes(g, d), ol.lanes(w.expand(rows, d), d), ol.lanes(xh, d)
    gw = _mul(g, w)
    gwl = ol.lanes(gw, d)
    s1 = _lane_chain(lambda c, j: (gl[:, c, :, j], wl[:, c, :, j]), d, fused=grouping == 1)
    s2 = _lane_chain(lambda c, j: (gwl[:, c, :, j], xl[:, c, :, j]), d, fused=True)
    c1 = ol.round_f32(s1 / (64 if mutant == "c1_divided_by_64" else d))[:, None]
    c2 = ol.round_f32(s2 / d)[:, None]
    if mutant == "xhat_c2_dropped":
        c2 = 0 * c2
    if grouping == 0:
        t = add_exact(add_exact(gw, -c1), -_mul(xh, c2))
    else:
        t = fmaf_exact(-xh, c2, fmaf_exact(g, w, -c1))
    dx = _mul(rstd[:, None], t)
    if dtype == BF16:
        dx = ol.round_bf16(dx)
    return dict(y=y.to(dtype), stats=stats, dx=dx.to(dtype), dweight=dweight.float(), dbias=dbias.float())


# (family, dtype, rows, D, relu): small shapes that reach both geometries, several blocks, idle wavefronts
CASES = [("gaussian", F32, 5, 256, False), ("gaussian", BF16, 5, 1024, True), ("gaussian", BF16, 65, 256, True),
         ("constant", BF16, 5, 256, True), ("near_constant", F32, 5, 256, False), ("near_constant", BF16, 5, 512, False),
         ("offset", F32, 5, 256, False), ("offset", BF16, 5, 512, True), ("near_zero", F32, 65, 256, True),
         ("near_zero", BF16, 5, 1024, True)]
WRAP = ("gaussian", F32, 2049, 256, True)                    # the smallest row count at which a wavefront walks twice

MUTANTS = ["eps_dropped", "eps_after_sqrt", "one_pass_variance", "divisor_d_minus_1", "mean_first_chunk",
           "y_lanes_permuted", "weight_bias_v8_map", "mask_z_ge_0", "mask_from_float64_z", "bf16_store_truncates",
           "bf16_halves_swapped", "xhat_c2_dropped", "c1_divided_by_64", "wave_left_out_of_fold",
           "last_partial_row_left_out", "partial_row_counted_twice", "dweight_dbias_swapped", "rows_past_2048_skipped",
           "rstd_stored_as_variance"]

_cases = {}


def _case(spec):
    if spec not in _cases:
        family, dtype, rows, d, _ = spec
        _cases[spec] = lc.make_case(family, dtype, rows, d)
    return _cases[spec]


@pytest.mark.parametrize("grouping", [0, 1], ids=["separate", "contracted"])
@pytest.mark.parametrize("spec", CASES + [WRAP], ids=lambda s: f"{s[0]}-{str(s[1])[6:]}-{s[2]}x{s[3]}-relu{int(s[4])}")
def test_checks_accept_the_fp32_emulation(spec, grouping):
    case = _case(spec)
    ratios = lc.run_checks(case, emulate(case, spec[4], grouping=grouping), spec[4])
    print("\n" + lc.fmt(ratios))
    assert lc.passes(ratios), lc.fmt(ratios)
    for k in ("stats.mean", "forward.y", "mask.mask", "backward.dweight", "backward.dbias"):
        assert ratios[k] == 0.0, k                                         # bit-equal, not merely within a bound


@pytest.mark.parametrize("mutant", MUTANTS)
def test_checks_reject_the_mutant(mutant):
    specs = [WRAP] if mutant == "rows_past_2048_skipped" else CASES
    caught = {}
    for spec in specs:
        case = _case(spec)
        ratios = lc.run_checks(case, emulate(case, spec[4], mutant=mutant), spec[4])
        bad = {k: v for k, v in ratios.items() if not v <= 1.0}
        if bad:
            caught[f"{spec[0]}-{str(spec[1])[6:]}-{spec[2]}x{spec[3]}"] = bad
    print(f"\n{mutant}: " + "; ".join(f"{k}: {lc.fmt(v)}" for k, v in caught.items()))
    assert caught, f"{mutant} passed every check on every family"


def test_a_nan_or_a_wrong_shape_is_an_infinite_ratio():
    spec = CASES[0]
    case = _case(spec)
    out = emulate(case, spec[4])
    for key in ("y", "dx", "dweight", "dbias", "stats"):
        bad = dict(out)
        bad[key] = out[key].clone()
        bad[key].view(-1)[3] = float("nan")
        assert lc.worst(lc.run_checks(case, bad, spec[4])) == float("inf"), key
        bad[key] = out[key][..., :-1]
        assert lc.worst(lc.run_checks(case, bad, spec[4])) == float("inf"), key


# ------------------------------------------------------------------------------------------- wrapper refusals

def _good(d=256, rows=3, dtype=F32):
    return dict(x=torch.zeros(rows, d, dtype=dtype), dy=torch.zeros(rows, d, dtype=dtype), weight=torch.ones(d),
                bias=torch.zeros(d), stats=torch.zeros(rows, 2))


REFUSALS = {
    "x_not_contiguous": (lambda a: a.update(x=torch.zeros(256, 3).t()), "x must be contiguous"),
    "x_float64": (lambda a: a.update(x=a["x"].double()), "x must be float32 or bfloat16"),
    "weight_bf16": (lambda a: a.update(weight=a["weight"].bfloat16()), "weight must be torch.float32"),
    "bias_float64": (lambda a: a.update(bias=a["bias"].double()), "bias must be torch.float32"),
    "weight_strided": (lambda a: a.update(weight=torch.ones(512)[::2]), "weight must be contiguous"),
    "bias_strided": (lambda a: a.update(bias=torch.ones(512)[::2]), "bias must be contiguous"),
    "weight_length": (lambda a: a.update(weight=torch.ones(512)), "weight must be"),
    "bias_length": (lambda a: a.update(bias=torch.ones(255)), "bias must be"),
}
BACKWARD_REFUSALS = {
    "dy_dtype": (lambda a: a.update(dy=a["dy"].bfloat16()), "dy must be torch.float32"),
    "dy_shape": (lambda a: a.update(dy=torch.zeros(2, 256)), "dy must be"),
    "dy_not_contiguous": (lambda a: a.update(dy=torch.zeros(256, 3).t()), "dy must be contiguous"),
    "stats_dtype": (lambda a: a.update(stats=a["stats"].double()), "stats must be torch.float32"),
    "stats_shape": (lambda a: a.update(stats=torch.zeros(2, 3)), "stats must be"),
    "stats_flat": (lambda a: a.update(stats=torch.zeros(6)), "stats must be"),
    "stats_not_contiguous": (lambda a: a.update(stats=torch.zeros(3, 4)[:, ::2]), "stats must be contiguous"),
}


@pytest.mark.parametrize("name", list(REFUSALS))
def test_wrappers_refuse_bad_arguments_before_any_device_work(name):
    import seld_native
    change, message = REFUSALS[name]
    a = _good()
    change(a)
    with pytest.raises(seld_native.SeldNativeError, match=message):
        seld_native.layernorm_forward(a["x"], a["weight"], a["bias"], 1e-5, False)
    with pytest.raises(seld_native.SeldNativeError, match=message):
        seld_native.layernorm_backward(a["x"], a["dy"] if name != "x_float64" else a["dy"].double(), a["weight"],
                                       a["bias"], a["stats"], False)


@pytest.mark.parametrize("name", list(BACKWARD_REFUSALS))
def test_backward_wrapper_refuses_bad_dy_and_stats(name):
    import seld_native
    change, message = BACKWARD_REFUSALS[name]
    a = _good()
    change(a)
    with pytest.raises(seld_native.SeldNativeError, match=message):
        seld_native.layernorm_backward(a["x"], a["dy"], a["weight"], a["bias"], a["stats"], False)


def test_well_formed_cpu_arguments_get_as_far_as_the_device_check():
    """The refusals above are about the arguments: the same call with good ones fails only for want of a GPU."""
    import seld_native
    a = _good()
    with pytest.raises(seld_native.SeldNativeError, match="ROCm device"):
        seld_native.layernorm_forward(a["x"], a["weight"], a["bias"], 1e-5, False)
    with pytest.raises(seld_native.SeldNativeError, match="ROCm device"):
        seld_native.layernorm_backward(a["x"], a["dy"], a["weight"], a["bias"], a["stats"], False)
