"""Cases for and assertions on the outputs of the first encoder block's kernels (csrc/convfirst.hip), shared by the
CPU tests (which feed them an emulation and named mutants, tests/test_convfirst_oracle_cpu.py) and the GPU tests
(which feed them the kernels' outputs, tests/test_convfirst_parity_gpu.py).  Reference: oracle/convfirst.py on
oracle/convtail.py, float64 on the CPU.

The kernels never store the convolution output x1, so an element-wise replay needs inputs on which x1 is known to the
bit.  ``make_case`` builds two families whose 36-term fp32 accumulation is exact in ANY order, so that
x1 = round_bf16(float64 conv) whatever the order inside the matrix instruction:

  integer   x in {-2..2}, every output channel of w has exactly 8 entries of +-1 among its 36, dy in {-4..4}.
            |x1| <= 16 is an integer, so nothing is rounded, and every fp32 partial sum of x1, x1^2, dz and dz x1 is an
            integer below 2^24 (rows per accumulator < 2^16): all statistics are exact, ties are frequent.
  dyadic    x = k / 16 (|k| <= 32), w = m / 64 (|m| <= 16), dy in {-4..4}.  Products are multiples of 2^-10 and
            |sum| <= 36 * 2 * 0.25 = 18, i.e. below 2^15 such multiples: the accumulation is exact, the operands use
            the whole bf16 mantissa and x1 is really rounded (most outputs need more than 8 bits).

Every check returns {name: worst error / bound} and passes at <= 1, with the NaN / infinity handling of
tests/tail_checks.py (``ratio``, ``mismatch``).  No measured constant enters a bound:

  u = 2^-24     the relative error of one fp32 rounding
  rho           the store rounding of dw: 2^-8 for bf16, 0 for fp32
  D             the longest fp32 addition chain a term of a statistic passes through: a wave adds 64 positions per
                chunk it walks (4 tiles of 16, two K = 32 matrix instructions), ceil(chunks / workgroups) chunks, and
                the four waves are added in order (+ 3).  The workgroups' partials are combined in double.
  D_w           the same for the weight gradient, whose slots are summed in fp32:  D + ceil(slots / 16) + 15
                (16 row sums of every 16th slot, then the 16 row sums in order)
"""
import torch

import tail_checks as tc
from oracle import convfirst as ocf
from oracle import convtail as oc

F64 = torch.float64
U = tc.U
RHO = tc.RHO
AMBIGUOUS_MARGIN = 2.0 ** -20
AMBIGUOUS_CAP = 0.01
MAX_GROUPS = 512                       # kCfMaxGroups


# ------------------------------------------------------------------------------------------------- cases

def make_case(family, shape, seed=0, momentum=0.1):
    """Inputs of one block call as CPU tensors: x [B, 4, T, F], w [64, 4, 3, 3], dy [B, 64, T, F / 2], all bf16 and in
    standard strides; gamma in [0.5, 1.5), beta ~ 0.3 N(0, 1); running statistics started from random values."""
    b, t, f = shape
    g = torch.Generator().manual_seed(7919 * seed + 1000 * b + 10 * t + f + (0 if family == "integer" else 500000))
    if family == "integer":
        x = torch.randint(-2, 3, (b, 4, t, f), generator=g).to(F64)
        w = torch.zeros(64, 36, dtype=F64)
        for co in range(64):
            taps = torch.randperm(36, generator=g)[:8]
            w[co, taps] = (torch.randint(0, 2, (8,), generator=g) * 2 - 1).to(F64)
        w = w.view(64, 4, 3, 3)
    elif family == "dyadic":
        x = torch.randint(-32, 33, (b, 4, t, f), generator=g).to(F64) / 16
        w = torch.randint(-16, 17, (64, 4, 3, 3), generator=g).to(F64) / 64
    else:
        raise ValueError(family)
    dy = torch.randint(-4, 5, (b, 64, t, f // 2), generator=g)
    case = dict(family=family, shape=(b, t, f), x=x.to(torch.bfloat16), w=w.to(torch.bfloat16), dy=dy.to(torch.bfloat16),
                weight=torch.rand(64, generator=g) + 0.5, bias=torch.randn(64, generator=g) * 0.3,
                rm0=torch.randn(64, generator=g), rv0=torch.rand(64, generator=g) + 0.5, eps=1e-5, momentum=momentum)
    assert torch.equal(case["x"].to(F64), x) and torch.equal(case["w"].to(F64), w)      # exact in bf16
    return case


EDGES = ["last_row_of_clip_0", "first_column", "last_column"]


def edge_case(family, shape, edge, seed=4):
    """A case whose x is zero except in the last time row of clip 0, or in the first / last frequency column: whatever
    the kernels read across a clip boundary or a frequency edge then shows in outputs that zero input alone explains."""
    b, t, f = shape
    case = make_case(family, shape, seed=seed)
    keep = torch.zeros(b, 4, t, f, dtype=torch.bool)
    if edge == "last_row_of_clip_0":
        keep[0, :, t - 1, :] = True
    elif edge == "first_column":
        keep[:, :, :, 0] = True
    elif edge == "last_column":
        keep[:, :, :, f - 1] = True
    else:
        raise ValueError(edge)
    case["x"] = torch.where(keep, case["x"], torch.zeros((), dtype=torch.bfloat16))
    assert case["x"].abs().sum() > 0
    return case


def rows_of(t):
    """[B, C, T, F] -> [B T F, C] in channels-last row order."""
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1]).contiguous()


def reference(case):
    """x1 [rows, 64] (rounded, float64), im2col(x) [rows, 36] and dy [rows / 2, 64] of a case, computed once."""
    if "_ref" not in case:
        case["_ref"] = dict(x1=ocf.x1(case["x"], case["w"]), cols=ocf.im2col(case["x"]), dy=rows_of(case["dy"]).to(F64))
    return case["_ref"]


def geometry(shape, cus):
    """The kernels' plan (cf_geometry / cf_groups) and the chain depths D, D_w that follow from it."""
    b, t, f = shape
    tc_rows = 256 // f
    per_clip = -(-t // tc_rows)
    chunks = b * per_clip
    groups = min(2 * cus, MAX_GROUPS, chunks)
    per_group = -(-chunks // groups)
    d = 64 * per_group + 3
    return dict(rows_per_chunk=tc_rows, chunks_per_clip=per_clip, chunks=chunks, groups=groups, per_group=per_group,
                D=d, D_w=d + -(-groups // 16) + 15)


# ------------------------------------------------------------------------------------------------- checks

def check_stats(case, ref, geom, out):
    """Coefficients, statistics and running statistics.

    a       bit-equal to fl32(weight * invstd_kernel): one fp32 multiplication of two fp32 numbers.
    b       bit-equal to fl32(bias - mean_k a_k) with the product fused or rounded first (either is a legal compilation).
    invstd  within 1 fp32 ulp of the float64 1 / sqrt(var + eps).
    running_mean / running_var   within 1 fp32 ulp of the float64 blend from rm0 / rv0.
    mean    integer family: the partial sums are exact and combined in double, so bit-equal to fl32(float64 mean).
            dyadic family: |mean - ref| <= u |ref| + D u mean|x|   (chain of D fp32 additions, the rest in double) and,
            with var recovered from the returned invstd (relative error 2 u + u^2 < 3 u of var + eps),
            |var - ref| <= 3 u (var + eps) + D u mean(x^2) + 2 |mean| D u mean|x|   (the products x x are exact)."""
    eps, momentum = tc.c_float(case["eps"]), tc.c_float(case["momentum"])
    x1 = ref["x1"]
    st = ocf.stats(x1, case["weight"], case["bias"], eps, case["rm0"], case["rv0"], momentum)
    mi, ss = out["mean_invstd"], out["scale_shift"]
    res = {"finite": 0.0 if tc.finite(mi, ss, out["running_mean"], out["running_var"]) else float("inf")}
    if mi.shape != (2, 64) or ss.shape != (2, 64):
        return {"finite": float("inf")}
    mean_k, invstd_k, a_k, b_k = mi[0].to(F64), mi[1].to(F64), ss[0].to(F64), ss[1].to(F64)
    w64, bias64 = case["weight"].to(F64), case["bias"].to(F64)
    res["a"] = tc.mismatch(ss[0], ocf.f32(w64 * invstd_k))
    fused = tc.mismatch(ss[1], oc.fmaf_exact(-mean_k, a_k, bias64))
    unfused = tc.mismatch(ss[1], ocf.f32(bias64 - ocf.f32(mean_k * a_k)))
    res["b"] = min(fused, unfused)
    ref_invstd = 1.0 / torch.sqrt(st["var"] + eps)
    res["invstd"] = tc.ratio((invstd_k - ref_invstd).abs(), tc.ulp32(ref_invstd))
    res["running_mean"] = tc.ratio((out["running_mean"].to(F64) - st["running_mean"]).abs(), tc.ulp32(st["running_mean"]))
    res["running_var"] = tc.ratio((out["running_var"].to(F64) - st["running_var"]).abs(), tc.ulp32(st["running_var"]))
    mean64 = x1.mean(0)
    if case["family"] == "integer":
        res["mean"] = tc.mismatch(mi[0], ocf.f32(mean64))
    else:
        d = geom["D"]
        abs1, m2 = x1.abs().mean(0), (x1 * x1).mean(0)
        res["mean"] = tc.ratio((mean_k - mean64).abs(), U * mean64.abs() + d * U * abs1)
        var_bound = 3 * U * (st["var"] + eps) + d * U * m2 + 2 * mean64.abs() * d * U * abs1
        res["var"] = tc.ratio((invstd_k ** -2 - eps - st["var"]).abs(), var_bound)
    return res


def ambiguous(rep):
    """Mask of the dx1 elements whose bf16 rounding the replay cannot vouch for: the fp32 value before the rounding
    lies within 2^-20 (|a dz| + |q x| + |p|) of a bf16 rounding midpoint.  The kernel forms p and q from double sums
    that the replay reproduces only to double rounding, so either may differ by one fp32 ulp: 2^-23 (|p| + |q x|) on
    the value, plus a re-rounding of each of the two fused multiply-adds, 2^-24 (|q x| + |p|) and 2^-24 |value| --
    under 2^-21 of the magnitude sum; the margin is twice that.
    -> (mask, one bf16 ulp at each element)."""
    pre = rep["pre"]
    bits = pre.to(torch.float32).contiguous().view(torch.int32)
    off = ((bits & 0xFFFF) - 0x8000).abs().to(F64)                       # fp32 ulps to the midpoint of the bf16 interval
    ulp = tc.ulp32(pre)
    mag = (rep["a"] * rep["dz"]).abs() + (rep["q"] * rep["x"]).abs() + rep["p"].abs()
    return off * ulp <= AMBIGUOUS_MARGIN * mag, ulp * 65536.0


def check_backward(case, ref, geom, out, fwd=None):
    """dbeta, dgamma and every element of dW against the replay from the kernel's own a, b, mean, invstd.

    dbeta   bit-equal to fl32(sum dz): dz is integer-valued, every partial sum exact.
    dgamma  integer family: sum dz x is exact too, and (sum dz x - mean sum dz) invstd is formed in double, so within
            1 fp32 ulp of that expression on the kernel's mean / invstd; dyadic: within (D + 4) u sum|dz xhat|.
    dw      |dw - ref| <= rho |ref| + D_w u S + A:  S = |dx1|^T |im2col(x)| the magnitude sum, A = the sum over the
            ambiguous dx1 elements (``ambiguous``) of one bf16 ulp times |im2col|.  dw.ambiguous reports the share
            of ambiguous elements over the 1 % allowed."""
    mi, ss = out["mean_invstd"], out["scale_shift"]
    names = ("dbeta", "dgamma", "dw", "dw.ambiguous")
    if not tc.finite(mi, ss) or mi.shape != (2, 64) or ss.shape != (2, 64):
        return {k: float("inf") for k in names}
    mean_k, invstd_k, a_k, b_k = mi[0].to(F64), mi[1].to(F64), ss[0].to(F64), ss[1].to(F64)
    x1, cols = ref["x1"], ref["cols"]
    rep = ocf.backward(x1, cols, ref["dy"], a_k, b_k, mean_k, invstd_k, fwd=fwd)
    rep.update(a=a_k, x=x1)
    res = {"dbeta": tc.mismatch(out["dbeta"], ocf.f32(rep["s_dz"]))}
    err = (out["dgamma"].to(F64) - rep["s_dzx"]).abs()
    if case["family"] == "integer":
        res["dgamma"] = tc.ratio(err, tc.ulp32(rep["s_dzx"]))
    else:
        res["dgamma"] = tc.ratio(err, (geom["D"] + 4) * U * rep["mag_dzx"])
    mask, ulp16 = ambiguous(rep)
    res["dw.ambiguous"] = float(mask.to(F64).mean()) / AMBIGUOUS_CAP
    amb = ((ulp16 * mask).t() @ cols.abs()).view(64, 4, 3, 3)
    dw = out["dw"]
    if tuple(dw.shape) != (64, 4, 3, 3):
        res["dw"] = float("inf")
        return res
    bound = RHO[dw.dtype] * rep["dW"].abs() + geom["D_w"] * U * rep["S"] + amb
    res["dw"] = tc.ratio((dw.to(F64) - rep["dW"]).abs(), bound)
    return res


def run_checks(case, out, cus=256):
    """Every check on one set of outputs -- dict: y [rows / 2, 64] bf16, mean_invstd [2, 64], scale_shift [2, 64],
    running_mean, running_var, dw [64, 4, 3, 3] (bf16 or fp32), dgamma, dbeta -- for a device with ``cus`` compute
    units -> {"mean": ratio, "y": ..., "dw": ..., ...}.  y is compared bit for bit on every element with the replay of
    the tail from the kernel's own scale_shift (tail_checks.check_forward, mode 2)."""
    ref, geom = reference(case), geometry(case["shape"], cus)
    ratios = check_stats(case, ref, geom, out)
    fw, fwd = tc.check_forward(ref["x1"], None, out["scale_shift"], 2, out["y"])
    ratios.update(fw)
    ratios.update(check_backward(case, ref, geom, out, fwd))
    return ratios


# ------------------------------------------------------------------------------------------------- premises

def fp32_sums_exact(v):
    """True when summing v [rows, C] (float64 values representable in fp32) down the rows in fp32 gives the float64
    sum at every step of two different orders: forward, and in a fixed shuffled order.  Values of one sign pattern
    aside, an order-independent fp32 sum needs every partial sum representable, which is what the two walks show."""
    v = v.to(F64)
    if not torch.equal(v.to(torch.float32).to(F64), v):
        return False
    perm = torch.randperm(v.shape[0], generator=torch.Generator().manual_seed(1))
    for order in (v, v[perm]):
        if not torch.equal(torch.cumsum(order.to(torch.float32), 0).to(F64), torch.cumsum(order, 0)):
            return False
    return True


def premises(case):
    """What the families promise, measured on a case: conv_exact (the 36 products of every output, added in fp32 in
    two orders, give the float64 sum at every step), sums_exact (the same for x1, x1^2, dz and dz x1 down the rows),
    rounded (share of conv outputs that are not bf16 numbers), tied (share of positive pooled pairs whose two bins are
    equal), dead (share of pooled outputs that are 0)."""
    ref = reference(case)
    x1 = ref["x1"]
    w36 = case["w"].to(F64).reshape(64, 36)
    n = min(x1.shape[0], 512)
    prod = ref["cols"][:n, None, :] * w36[None, :, :]                           # [n, 64, 36] exact products
    conv_exact = fp32_sums_exact(prod.permute(2, 0, 1).reshape(36, -1))
    st = ocf.stats(x1, case["weight"], case["bias"], tc.c_float(case["eps"]), case["rm0"], case["rv0"],
                   tc.c_float(case["momentum"]))
    dz, fwd = ocf.route(x1, ref["dy"], st["a"], st["b"])
    sums_exact = all(fp32_sums_exact(v) for v in (x1, x1 * x1, dz, dz * x1))
    z0, z1 = fwd["z"][0::2], fwd["z"][1::2]
    positive = fwd["y"] > 0
    return dict(conv_exact=conv_exact, sums_exact=sums_exact,
                rounded=float((ocf.conv(case["x"], case["w"]) != x1).to(F64).mean()),
                tied=float(((z0 == z1) & positive).sum()) / max(int(positive.sum()), 1),
                dead=float((fwd["y"] == 0).to(F64).mean()))


worst, passes, fmt = tc.worst, tc.passes, tc.fmt
