"""CPU pins of the float64 oracle of the first encoder block (oracle/convfirst.py) and of the checks built on it
(tests/convfirst_checks.py):

  * with rounding switched off the oracle equals the stock float64 Conv2d -> BatchNorm2d -> ReLU -> MaxPool2d((1, 2))
    and its autograd;
  * the two input families keep their promises (exact fp32 sums, frequent ties, really rounded outputs);
  * the checks accept a restatement of the seven kernels' arithmetic and reject every deliberately wrong variant.
"""
import pytest
import torch
import torch.nn as nn

import convfirst_checks as cc
import tail_checks as tc
from oracle import convfirst as ocf
from oracle import convtail as oc

F64 = torch.float64
BF16 = torch.bfloat16

# the small shapes of tests/test_convfirst_parity_gpu.py
SHAPES = [(2, 3, 16), (2, 11, 32), (3, 5, 64), (2, 3, 128), (2, 3, 256), (1, 1, 16), (1, 1, 256), (3, 17, 16)]
FAMILIES = ["integer", "dyadic"]


# ------------------------------------------------------------------------------------------- stock-module pin

def _close(got, want, name):
    err = (got - want).abs().max().item()
    assert err <= 1e-11 * (want.abs().max().item() + 1e-30), (name, err)


@pytest.mark.parametrize("shape", [(2, 3, 16), (3, 5, 8), (1, 4, 6)])
def test_unrounded_oracle_equals_stock_float64_modules(shape):
    b, t, f = shape
    g = torch.Generator().manual_seed(10 * t + f)
    x = torch.randn(b, 4, t, f, generator=g, dtype=F64)
    conv = nn.Conv2d(4, 64, 3, padding=1, bias=False).double()
    bn = nn.BatchNorm2d(64, momentum=0.25).double().train()
    with torch.no_grad():
        conv.weight.copy_(torch.randn(64, 4, 3, 3, generator=g, dtype=F64) * 0.3)
        bn.weight.copy_(torch.rand(64, generator=g, dtype=F64) + 0.5)
        bn.bias.copy_(torch.randn(64, generator=g, dtype=F64) * 0.3)
        bn.running_mean.copy_(torch.randn(64, generator=g, dtype=F64))
        bn.running_var.copy_(torch.rand(64, generator=g, dtype=F64) + 0.5)
    rm0, rv0 = bn.running_mean.clone(), bn.running_var.clone()
    y = nn.MaxPool2d((1, 2))(torch.relu(bn(conv(x))))
    dy = torch.randn(y.shape, generator=g, dtype=F64)
    y.backward(dy)

    w = conv.weight.detach()
    x1 = ocf.x1(x, w, F64)
    _close(x1, cc.rows_of(conv(x).detach()), "x1")
    _close((ocf.im2col(x) @ w.reshape(64, 36).t()), x1, "im2col")
    st = ocf.stats(x1, bn.weight.detach(), bn.bias.detach(), bn.eps, rm0, rv0, 0.25, F64)
    _close(st["running_mean"], bn.running_mean, "running_mean")
    _close(st["running_var"], bn.running_var, "running_var")
    rep = ocf.backward(x1, ocf.im2col(x), cc.rows_of(dy), st["a"], st["b"], st["mean"], st["invstd"], F64)
    _close(rep["fwd"]["y"], cc.rows_of(y.detach()), "y")
    _close(rep["dbeta"], bn.bias.grad, "dbeta")
    _close(rep["dgamma"], bn.weight.grad, "dgamma")
    _close(rep["dW"], conv.weight.grad, "dW")
    assert (rep["S"] >= rep["dW"].abs() * (1 - 1e-12)).all()


# ------------------------------------------------------------------------------------------- the families' premises

@pytest.mark.parametrize("shape", SHAPES)
def test_integer_family_is_exact_and_full_of_ties(shape):
    case = cc.make_case("integer", shape)
    w = case["w"].to(F64).reshape(64, 36)
    assert bool(((w.abs() == 1).sum(1) == 8).all()) and bool(((w == 0).sum(1) == 28).all())
    assert case["x"].to(F64).abs().max() <= 2 and case["dy"].to(F64).abs().max() <= 4
    p = cc.premises(case)
    print(f"\ninteger {shape}: {p}")
    assert p["conv_exact"] and p["sums_exact"]
    assert p["rounded"] == 0.0
    assert cc.reference(case)["x1"].abs().max() <= 16
    if shape[1] * shape[2] >= 48:                                # a few hundred pairs per channel: the share is a share
        assert p["tied"] >= 0.01 and p["dead"] > 0.05


@pytest.mark.parametrize("shape", SHAPES)
def test_dyadic_family_is_exact_and_really_rounded(shape):
    case = cc.make_case("dyadic", shape)
    x, w = case["x"].to(F64), case["w"].to(F64)
    assert torch.equal((x * 16).round(), x * 16) and x.abs().max() <= 2
    assert torch.equal((w * 64).round(), w * 64) and w.abs().max() <= 0.25
    p = cc.premises(case)
    print(f"\ndyadic {shape}: {p}")
    assert p["conv_exact"]
    assert p["rounded"] >= 0.40


# ------------------------------------------------------------------------------------------- emulation and mutants

def _conv_rows(x, w):
    return oc.round_bf16(ocf.conv(x, w))


def _mutated_x1(case, mutant):
    x, w = case["x"].to(F64), case["w"].to(F64)
    b, c, t, f = x.shape
    if mutant == "clip_bleed":                                   # the padded rows above / below a clip hold the neighbour's
        return _conv_rows(x.permute(1, 0, 2, 3).reshape(1, c, b * t, f), w)
    if mutant == "freq_wrap":                                    # no zero column: f = -1 is the previous row's last bin
        flat = torch.nn.functional.pad(x.reshape(b, c, t * f), (f + 1, f + 1))
        out = torch.zeros(b, 64, t * f, dtype=F64)
        for r in range(3):
            for s in range(3):
                shift = (r - 1) * f + (s - 1)
                win = flat[:, :, f + 1 + shift: f + 1 + shift + t * f]
                out += torch.einsum("oc,bcn->bon", w[:, :, r, s], win)
        return oc.round_bf16(out.permute(0, 2, 1).reshape(-1, 64).contiguous())
    if mutant == "taps_transposed":
        return _conv_rows(x, w.transpose(2, 3))
    return _conv_rows(x, w)


def emulate(case, mutant=None, cus=256, dw_dtype=BF16):
    """The seven kernels' outputs restated on the CPU from oracle/convfirst.py: the statistics combined in double from
    (here: exact) sums and stored as fp32, the element-wise stages as fp32 fused multiply-adds with bf16 rounding, the
    weight gradient as an fp32 matrix product of the bf16 dx1 and the im2col of x.  ``mutant`` names one deliberate
    defect.  -> dict of the outputs in their dtypes."""
    b, t, f = case["shape"]
    geom = cc.geometry(case["shape"], cus)
    eps, momentum = tc.c_float(case["eps"]), tc.c_float(case["momentum"])
    x1 = _mutated_x1(case, mutant)
    cols, dy = cc.reference(case)["cols"], cc.reference(case)["dy"]
    rows = x1.shape[0]
    row = torch.arange(rows)
    tt, bb = (row // f) % t, row // (t * f)
    group = (bb * geom["chunks_per_clip"] + tt // geom["rows_per_chunk"]) % geom["groups"]
    ragged_last = (tt == t - 1) & (t % geom["rows_per_chunk"] != 0)            # last time row of a ragged chunk
    one = torch.ones(rows, 1, dtype=F64)
    keep_stats, keep_dw = one.clone(), one.clone()
    if mutant == "ragged_row_stats":
        keep_stats[ragged_last] = 0
    if mutant == "ragged_row_dw":
        keep_dw[ragged_last] = 0
    if mutant == "slot_dropped_stats":
        keep_stats[group == geom["groups"] - 1] = 0
    if mutant == "slot_dropped_dw":
        keep_dw[group == geom["groups"] - 1] = 0
    if mutant == "position_dropped":
        keep_dw[rows // 2] = 0
    n = rows
    if mutant == "n_counts_padded":
        n = b * geom["chunks_per_clip"] * geom["rows_per_chunk"] * f

    fin = ocf.finalise((x1 * keep_stats).sum(0), (x1 * x1 * keep_stats).sum(0), n, case["weight"], case["bias"], eps,
                       case["rm0"], case["rv0"], momentum)
    a, bcoef, mean, invstd = fin["a"], fin["b"], fin["mean"], fin["invstd"]

    zero = torch.zeros((), dtype=F64)
    zu = oc.fmaf_exact(x1, a, bcoef)
    z = oc.round_bf16(zu)
    zc = zu if mutant == "unrounded" else z                                     # what the comparisons see
    r0, r1 = torch.where(zc[0::2] > 0, zc[0::2], zero), torch.where(zc[1::2] > 0, zc[1::2], zero)
    second = r1 >= r0 if mutant == "tie_second" else r1 > r0
    m = torch.where(second, r1, r0)
    y = oc.round_bf16(m).to(BF16)
    passed = torch.ones_like(m, dtype=torch.bool) if mutant == "relu_gate_dropped" else m > 0
    dz = torch.zeros_like(x1)
    dz[0::2] = torch.where(passed & ~second, dy, 0.0)
    dz[1::2] = torch.where(passed & second, dy, 0.0)

    bw = ocf.bwd_final((dz * keep_stats).sum(0), (dz * x1 * keep_stats).sum(0), n, a, mean, invstd)
    dx1, _ = ocf.dx1_of(x1, dz, a, bw["p"], bw["q"])
    dw = ((dx1 * keep_dw).to(torch.float32).t() @ cols.to(torch.float32)).view(64, 4, 3, 3)
    if mutant == "taps_transposed_dw":
        dw = dw.transpose(2, 3).contiguous()
    if mutant == "last_pooled_row_unwritten":
        y[-1] = 1.0
    f32 = lambda v: v.to(torch.float32)
    out = dict(y=y, mean_invstd=torch.stack([f32(mean), f32(invstd)]), scale_shift=torch.stack([f32(a), f32(bcoef)]),
               running_mean=f32(fin["running_mean"]), running_var=f32(fin["running_var"]), dw=dw.to(dw_dtype),
               dgamma=f32(bw["dgamma"]), dbeta=f32(bw["dbeta"]))
    if mutant and mutant.startswith("nan_"):                                     # one NaN in one output
        target = out[mutant[4:]]
        target[(1, 3) if target.dim() == 2 else ((5, 2, 1, 0) if target.dim() == 4 else 1)] = float("nan")
    return out


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("shape", SHAPES)
def test_checks_accept_the_unmutated_emulation(shape, family):
    for momentum, dw_dtype in ((0.1, BF16), (0.25, torch.float32)):
        case = cc.make_case(family, shape, momentum=momentum)
        ratios = cc.run_checks(case, emulate(case, dw_dtype=dw_dtype))
        print(f"\n{family} {shape} momentum {momentum}: {cc.fmt(ratios)}")
        assert cc.passes(ratios), cc.fmt(ratios)
        assert ratios["dw.ambiguous"] <= 1.0                     # the 1 % cap on ambiguous dx1 elements


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("shape", [(2, 5, 16), (2, 3, 64)])
@pytest.mark.parametrize("edge", cc.EDGES)
def test_checks_accept_the_emulation_on_the_edge_cases(edge, shape, family):
    """x zero except at one clip or frequency edge: most dx1 elements of a channel then share one value, so this is
    where the share of ambiguous elements could jump; it stays under the cap."""
    case = cc.edge_case(family, shape, edge)
    ratios = cc.run_checks(case, emulate(case))
    print(f"\n{family} {shape} {edge}: {cc.fmt(ratios)}")
    assert cc.passes(ratios), cc.fmt(ratios)


@pytest.mark.parametrize("family", FAMILIES)
def test_checks_accept_a_multi_chunk_walk(family):
    """2 compute units -> 4 workgroups for the 15 chunks of (3, 17, 64): four chunks per workgroup."""
    case = cc.make_case(family, (3, 17, 64))
    geom = cc.geometry(case["shape"], 2)
    assert (geom["chunks"], geom["groups"], geom["per_group"], geom["D"], geom["D_w"]) == (15, 4, 4, 259, 275)
    ratios = cc.run_checks(case, emulate(case, cus=2), cus=2)
    assert cc.passes(ratios), cc.fmt(ratios)


def test_chain_depths_follow_the_plan():
    g = cc.geometry((5, 211, 256), 256)                          # the walk at F = 256 on 256 compute units
    assert (g["chunks"], g["groups"], g["per_group"], g["D"], g["D_w"]) == (1055, 512, 3, 195, 242)
    g = cc.geometry((5, 821, 64), 256)
    assert (g["chunks"], g["groups"], g["per_group"]) == (1030, 512, 3)
    g = cc.geometry((2, 11, 32), 256)                            # one chunk per workgroup
    assert (g["rows_per_chunk"], g["chunks"], g["groups"], g["per_group"], g["D"], g["D_w"]) == (8, 4, 4, 1, 67, 83)


RAGGED = (2, 11, 32)                   # 8 rows per chunk: a full chunk and one of 3 rows per clip

# (mutant, family, shape, compute units, the checks that must reject it)
MUTANTS = [
    ("tie_second", "integer", RAGGED, 256, ["dw"]),
    ("unrounded", "dyadic", (3, 17, 64), 256, ["dw"]),
    ("relu_gate_dropped", "integer", RAGGED, 256, ["dbeta", "dgamma", "dw"]),
    ("relu_gate_dropped", "dyadic", RAGGED, 256, ["dbeta", "dgamma", "dw"]),
    ("ragged_row_stats", "integer", RAGGED, 256, ["mean", "invstd", "dbeta"]),
    ("ragged_row_stats", "dyadic", RAGGED, 256, ["mean", "var", "dbeta"]),
    ("ragged_row_dw", "integer", RAGGED, 256, ["dw"]),
    ("ragged_row_dw", "dyadic", (3, 17, 64), 2, ["dw"]),
    ("clip_bleed", "integer", RAGGED, 256, ["mean", "y", "dw"]),
    ("clip_bleed", "dyadic", (3, 17, 64), 2, ["mean", "y", "dw"]),
    ("freq_wrap", "integer", RAGGED, 256, ["mean", "y", "dw"]),
    ("freq_wrap", "dyadic", (2, 3, 256), 256, ["mean", "y", "dw"]),
    ("n_counts_padded", "integer", RAGGED, 256, ["mean", "invstd", "running_mean", "running_var"]),
    ("n_counts_padded", "dyadic", RAGGED, 256, ["mean", "var", "running_mean", "running_var"]),
    ("taps_transposed", "integer", RAGGED, 256, ["mean", "y", "dw"]),
    ("taps_transposed", "dyadic", RAGGED, 256, ["y", "dw"]),
    ("taps_transposed_dw", "integer", RAGGED, 256, ["dw"]),
    ("slot_dropped_stats", "integer", RAGGED, 256, ["mean", "dbeta"]),
    ("slot_dropped_dw", "integer", RAGGED, 256, ["dw"]),
    ("slot_dropped_dw", "dyadic", (3, 17, 64), 2, ["dw"]),
    ("position_dropped", "integer", RAGGED, 256, ["dw"]),
    ("position_dropped", "dyadic", (3, 17, 64), 2, ["dw"]),
    ("last_pooled_row_unwritten", "integer", RAGGED, 256, ["y"]),
    ("last_pooled_row_unwritten", "dyadic", (1, 1, 16), 256, ["y"]),
    # a single NaN: in an output, in a parameter gradient, in a coefficient (from which the replay would reproduce it)
    ("nan_y", "integer", RAGGED, 256, ["y"]),
    ("nan_dw", "dyadic", RAGGED, 256, ["dw"]),
    ("nan_dgamma", "integer", RAGGED, 256, ["dgamma"]),
    ("nan_dbeta", "dyadic", RAGGED, 256, ["dbeta"]),
    ("nan_scale_shift", "integer", RAGGED, 256, ["finite", "y", "dw"]),
    ("nan_mean_invstd", "dyadic", RAGGED, 256, ["finite", "dw", "dgamma"]),
    ("nan_running_mean", "integer", RAGGED, 256, ["finite", "running_mean"]),
    ("nan_running_var", "dyadic", RAGGED, 256, ["finite", "running_var"]),
]


@pytest.mark.parametrize("mutant,family,shape,cus,rejected_by", MUTANTS)
def test_checks_reject_every_mutant(mutant, family, shape, cus, rejected_by):
    case = cc.make_case(family, shape, seed=3)
    good = cc.run_checks(case, emulate(case, cus=cus), cus=cus)
    assert cc.passes(good), cc.fmt(good)
    bad = cc.run_checks(case, emulate(case, mutant, cus=cus), cus=cus)
    print(f"\n{mutant} {family} {shape}: {cc.fmt(bad)}")
    for name in rejected_by:
        assert not bad[name] <= 1.0, (mutant, name, cc.fmt(bad))
    assert not cc.passes(bad) and cc.worst(bad) > 1.0, (mutant, cc.fmt(bad))


@pytest.mark.parametrize("family", FAMILIES)
def test_a_nan_in_any_output_fails_the_pass_criterion(family):
    case = cc.make_case(family, (2, 3, 16), seed=11)
    for name in ("y", "dw", "dgamma", "dbeta", "mean_invstd", "scale_shift", "running_mean", "running_var"):
        bad = cc.run_checks(case, emulate(case, "nan_" + name))
        assert not cc.passes(bad) and cc.worst(bad) == float("inf"), (name, cc.fmt(bad))
