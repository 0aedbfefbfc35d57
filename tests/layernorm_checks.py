"""Assertions on the outputs of the fused LayerNorm [-> ReLU] kernels (csrc/layernorm.hip), shared by the CPU tests
(which feed them an fp32 emulation and its mutants) and the GPU tests (which feed them the kernels' outputs).
Reference: oracle/layernorm.py, float64 on the CPU.

Every check takes CPU tensors -- x, dy, y, dx ``[rows, D]`` in the kernel's dtype, weight / bias / dweight / dbias
``[D]`` fp32, stats ``[rows, 2]`` fp32 (mean, rstd) -- and returns {name: worst error / bound}; a check passes when
every ratio is <= 1.  A bit-equality check reports 0 or 1 + the number of differing elements.  A NaN or an infinity
anywhere gives an infinite ratio (``tail_checks.ratio`` / ``mismatch``).  Symbols:

  u = 2^-24        the relative error of one fp32 rounding;  gamma(n) = n u / (1 - n u)
  rho              the allowance for the output's store rounding: 2^-8 bf16, 0 fp32
  h = kChunks V + 6    additions between an element and its row sum (lane chain + butterfly)
  A = RSQRT_ULPS   the one allowance that is not derived: the distance of ``rsqrtf`` from the correctly rounded value
"""
import torch

from oracle import layernorm as ol
from tail_checks import F64, RHO, U, finite, fmt, mismatch, passes, ratio, ulp32, worst  # noqa: F401

# Worst |rstd - 1 / sqrt(var + eps)| / ulp over every parity case on the MI355X (tests/test_layernorm_parity_gpu.py
# prints it per case); the allowance is that plus one ulp, never more than 4.
RSQRT_MEASURED = 0.80
RSQRT_ULPS = min(RSQRT_MEASURED + 1.0, 4.0)

_SUB32 = 2.0 ** -149          # the smallest fp32 subnormal: the absolute error of a rounding that underflows
_SUB16 = 2.0 ** -134          # half the smallest bf16 subnormal


def gamma(n):
    return n * U / (1.0 - n * U)


def _bits_differ(a, b):
    return 0.0 if not bool((a != b).any()) else 1.0 + int((a != b).sum())


def rsqrt_distance(x, eps, stats):
    """Worst distance in fp32 ulps between the returned rstd and the float64 1 / sqrt of the replayed var + eps."""
    _, ve = ol.row_stats_replay(x.to(F64), eps, x.shape[1])
    ref = 1.0 / torch.sqrt(ve)
    return ratio((stats[:, 1].to(F64) - ref).abs(), ulp32(ref))


# ------------------------------------------------------------------------------------------------- statistics

def check_stats(x, eps, stats):
    """mean -- bit-equal to ``row_stats_replay`` (the kernel's own summation order).
    rstd -- within A ulps of the float64 1 / sqrt(v), v the replayed fp32 ``var + eps``.  A cannot be derived from
      this code; the installed HIP documentation carries no accuracy table, so it is measured: the worst distance over
      all parity cases on the MI355X is 0.792 ulp, recorded as RSQRT_MEASURED = 0.80, A = that + 1 = 1.8.
    mean_free, var_free -- independently of any order, against the float64 two-pass statistics m, s2:
        |mean - m|  <=  gamma(h) mean|x| =: Bm                       (h additions per element; the 1 / D is exact)
        |1 / rstd^2 - eps - s2|  <=  Bm^2 + gamma(h + 3) (s2 + Bm^2) + (2 + 4 A) u (s2 + Bm^2 + eps)
      Bm^2: the kernel centres on its own mean, mean((x - m')^2) = s2 + (m' - m)^2;  h + 3: x - m' is rounded once and
      squared (2 u), then h fused accumulations;  the eps addition is one rounding and A ulps (<= 2 A u relative) on
      rstd are 4 A u on its inverse square."""
    if stats.shape != (x.shape[0], 2) or not finite(stats):
        return {"mean": float("inf"), "rstd": float("inf"), "mean_free": float("inf"), "var_free": float("inf")}
    d = x.shape[1]
    x64 = x.to(F64)
    eps = ol.c_float(eps)
    mean_k, rstd_k = stats[:, 0].to(F64), stats[:, 1].to(F64)
    mean_r, ve = ol.row_stats_replay(x64, eps, d)
    ref = 1.0 / torch.sqrt(ve)
    out = {"mean": mismatch(stats[:, 0], mean_r),
           "rstd": ratio((rstd_k - ref).abs(), RSQRT_ULPS * ulp32(ref))}
    h = ol.sum_depth(d)
    m = x64.mean(1)
    s2 = ((x64 - m[:, None]) ** 2).mean(1)
    bm = gamma(h) * x64.abs().mean(1) + _SUB32
    bv = bm ** 2 + gamma(h + 3) * (s2 + bm ** 2) + (2 + 4 * RSQRT_ULPS) * U * (s2 + bm ** 2 + eps)
    out["mean_free"] = ratio((mean_k - m).abs(), bm)
    out["var_free"] = ratio((rstd_k ** -2 - eps - s2).abs(), bv)
    return out


# ------------------------------------------------------------------------------------------------- forward

def check_forward(x, weight, bias, stats, relu, y):
    """y equals ``forward_replay`` from the kernel's own returned statistics bit for bit, every element, the sign of a
    zero included (every operation between the statistics and the store is a single fp32 operation or an fmaf)."""
    if y.shape != x.shape or stats.shape != (x.shape[0], 2) or not finite(stats, y):
        return {"y": float("inf")}
    fwd = ol.forward_replay(x.to(F64), weight, bias, stats[:, 0], stats[:, 1], relu, y.dtype)
    return {"y": mismatch(y, fwd["y"])}


def check_mask(x, weight, bias, stats, relu, y):
    """With ReLU the backward pass recomputes the pre-activation; its mask ``fmaf(xhat, w, b) > 0`` must be the mask
    ``y > 0`` of the forward output the kernel actually stored, on every element (no element is excluded for being
    close to zero).  0 or 1 + the number of disagreements."""
    if not relu:
        return {"mask": 0.0}
    if y.shape != x.shape or stats.shape != (x.shape[0], 2) or not finite(stats):
        return {"mask": float("inf")}
    xh = ol.xhat_replay(x.to(F64), stats[:, 0], stats[:, 1])
    return {"mask": _bits_differ(ol.fmaf_exact(xh, weight.to(F64), bias.to(F64)) > 0, y.to(F64) > 0)}


# ------------------------------------------------------------------------------------------------- backward

def check_backward(x, dy, weight, bias, stats, relu, y, dx, dweight, dbias, rows_per_launch=None):
    """Gradients from the kernel's own statistics; with ReLU the float64 references use the mask ``y > 0`` of the
    kernel's own forward output, on every row.

    dweight, dbias -- bit-equal to ``backward_replay`` (wavefront chains, block fold, halving tree, groups).
    dweight_free, dbias_free -- independently of the order, against the float64 sums of the same masked terms
      t = g xhat (xhat the kernel's fp32 value) and t = g:
        |sum - ref|  <=  gamma(p + 2) sum|t|,   p = ceil(rows / rows_per_launch) + 3 + 5 + 16
      the additions on the longest path through the kernel's order; 2 for the product and slack.
    dx -- ref = rstd (g w - c1 - xhat c2), c1 = mean(g w), c2 = mean(g w xhat) in float64 from the same xhat, mask and
      statistics.  The kernel rounds g w (u), sums it over h additions (c1: gamma(h + 1) mean|g w| =: E1; c2 likewise,
      E2 = gamma(h + 1) mean|g w xhat|), rounds xhat c2, two subtractions and the product with rstd; a contraction of
      any of these into an FMA only removes a rounding.  Collecting at most 4 u on each term:
        |dx - ref|  <=  rstd (4 u (|g w| + |c1| + |xhat c2|) + E1 + |xhat| E2 + 4 * 2^-149)  +  rho |ref|  [+ 2^-134 bf16]
      (the last two absolute terms: roundings that underflow, and a bf16 store into the subnormal range)."""
    names = ("dweight", "dbias", "dweight_free", "dbias_free", "dx")
    d = x.shape[1]
    if (dx.shape != x.shape or dweight.shape != (d,) or dbias.shape != (d,) or stats.shape != (x.shape[0], 2)
            or y.shape != x.shape or not finite(stats)):
        return {k: float("inf") for k in names}
    x64, dy64, w64 = x.to(F64), dy.to(F64), weight.to(F64)
    rows = x64.shape[0]
    mean_k, rstd_k = stats[:, 0], stats[:, 1]
    rep = ol.backward_replay(x64, dy64, weight, bias, mean_k, rstd_k, relu, dx.dtype, rows_per_launch)
    out = {"dweight": mismatch(dweight, rep["dweight"]), "dbias": mismatch(dbias, rep["dbias"])}
    xh = rep["xhat"]
    g = torch.where(y.to(F64) > 0, dy64, torch.zeros((), dtype=F64)) if relu else dy64
    p = ol.column_depth(rows, rows_per_launch)
    t = g * xh
    out["dweight_free"] = ratio((dweight.to(F64) - t.sum(0)).abs(), gamma(p + 2) * t.abs().sum(0))
    out["dbias_free"] = ratio((dbias.to(F64) - g.sum(0)).abs(), gamma(p + 2) * g.abs().sum(0))
    h = ol.sum_depth(d)
    rstd = rstd_k.to(F64)[:, None]
    gw = g * w64
    c1, c2 = gw.mean(1, keepdim=True), (gw * xh).mean(1, keepdim=True)
    ref = rstd * (gw - c1 - xh * c2)
    e1 = gamma(h + 1) * gw.abs().mean(1, keepdim=True)
    e2 = gamma(h + 1) * (gw * xh).abs().mean(1, keepdim=True)
    bound = rstd.abs() * (4 * U * (gw.abs() + c1.abs() + (xh * c2).abs()) + e1 + xh.abs() * e2 + 4 * _SUB32) + \
        RHO[dx.dtype] * ref.abs() + (_SUB16 if dx.dtype == torch.bfloat16 else 0.0)
    out["dx"] = ratio((dx.to(F64) - ref).abs(), bound)
    return out


def run_checks(case, out, relu, rows_per_launch=None):
    """All four checks on one set of outputs (dict: y, stats, dx, dweight, dbias) -> {"stats.mean": ratio, ...}."""
    x, dy, w, b = case["x"], case["dy"], case["weight"], case["bias"]
    ratios = {}
    for name, res in (("stats", check_stats(x, case["eps"], out["stats"])),
                      ("forward", check_forward(x, w, b, out["stats"], relu, out["y"])),
                      ("mask", check_mask(x, w, b, out["stats"], relu, out["y"])),
                      ("backward", check_backward(x, dy, w, b, out["stats"], relu, out["y"], out["dx"], out["dweight"],
                                                  out["dbias"], rows_per_launch))):
        ratios.update({f"{name}.{k}": v for k, v in res.items()})
    return ratios


# ------------------------------------------------------------------------------------------------- cases

FAMILIES = ("gaussian", "constant", "near_constant", "offset", "near_zero")


def replay_rstd(x, eps):
    """(mean, rstd) of the replay with a correctly rounded reciprocal square root, fp32 values as float64."""
    mean, ve = ol.row_stats_replay(x.to(F64), eps, x.shape[1])
    return mean, ol.round_f32(1.0 / torch.sqrt(ve))


def make_case(family, dtype, rows, d, seed=0, eps=1e-5):
    """Inputs of one call as CPU tensors: x, dy [rows, D] in ``dtype``; weight, bias [D] fp32; eps.

    gaussian       the distribution of tests/test_layernorm_gpu.py: x = 3 n + 1.5 (fp32), 2 n (bf16)
    constant       every row one bf16-valued constant: x - mean is exactly 0
    near_constant  row variance within a factor 4 of eps on either side: fp32 0.5 + s n with s^2 = eps 4^[-0.8, 0.8];
                   bf16 0.5 + 2^-8 k, k uniform on {0..m-1}, m = 2..5 by row (variance (m^2 - 1) / 12 * 2^-16)
    offset         |mean| >> std: fp32 4096 + s n, s log-uniform in [0.01, 1]; bf16 64 + n
    near_zero      four distinct Gaussian rows repeated; column c is tuned to row pattern c % 4: bias = -fp32(xhat w)
                   from the replayed statistics, so the pre-activation there is the rounding residual of one product,
                   of either sign; every 16th column has w = 0 and bias = -0, which gives exactly -0 where xhat < 0 and
                   exactly +0 where xhat > 0 whatever the last bit of rstd"""
    g = torch.Generator().manual_seed(7919 * FAMILIES.index(family) + 31 * d + rows + seed)
    n = lambda *shape: torch.randn(*shape, generator=g)
    weight = n(d) * 0.5 + 1
    bias = n(d) * 0.2
    if family == "gaussian":
        x = n(rows, d) * 3 + 1.5 if dtype == torch.float32 else n(rows, d) * 2
    elif family == "constant":
        x = (n(rows, 1) * 4).bfloat16().float().expand(rows, d)
    elif family == "near_constant":
        if dtype == torch.float32:
            s = (eps * 4.0 ** (torch.rand(rows, 1, generator=g) * 1.6 - 0.8)).sqrt()
            x = 0.5 + s * n(rows, d)
        else:
            m = (torch.arange(rows) % 4 + 2).view(rows, 1)
            k = (torch.rand(rows, d, generator=g) * m).floor()
            k[:, 0], k[:, 1] = 0, (m - 1).view(-1)                  # every level span is present
            x = 0.5 + 2.0 ** -8 * k
    elif family == "offset":
        if dtype == torch.float32:
            x = 4096 + 10.0 ** (torch.rand(rows, 1, generator=g) * 2 - 2) * n(rows, d)
        else:
            x = 64 + n(rows, d)
    elif family == "near_zero":
        pat = n(4, d) * 3 + 1.5 if dtype == torch.float32 else n(4, d) * 2
        x = pat[torch.arange(rows) % 4]
    else:
        raise ValueError(family)
    x = x.to(dtype).contiguous()
    if family == "near_zero":
        pat64 = pat.to(dtype).to(F64)
        mean, rstd = replay_rstd(pat64, eps)
        xh = ol.xhat_replay(pat64, mean, rstd)
        col = torch.arange(d)
        tuned = xh[col % 4, col]
        bias = -(tuned * weight.double()).float()
        weight[::16] = 0.0
        bias[::16] = -0.0
    dy = n(rows, d).to(dtype)
    return dict(x=x, dy=dy, weight=weight.contiguous(), bias=bias.contiguous(), eps=eps)
