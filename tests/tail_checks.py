"""Assertions on the outputs of the fused BatchNorm tails (csrc/convtail.hip) and the depthwise Conv1d kernels
(csrc/dwconv.hip), shared by the CPU tests (which feed them emulations and mutants) and the GPU tests (which feed them
the kernels' outputs).  References: oracle/convtail.py and oracle/dwconv.py, float64 on the CPU.

Every check takes CPU tensors -- activations as [rows, C] in the kernel's dtype -- and returns {name: worst
error / bound}; a check passes when every ratio is <= 1 (``passes``).  A bit-equality check reports 0 or 1 + the number
of differing elements.  A NaN or an infinity anywhere -- in an output, a returned coefficient, an error or a bound --
is reported as an infinite ratio, never as a NaN that a comparison or ``max`` could drop.  No measured constant enters
a bound:

  u = 2^-24      the relative error of one fp32 rounding
  rho            the allowance for the output's store rounding: 2^-8 for bf16 (as tests/test_conv_dgrad_gpu.py), 0 fp32
  2e-5           this project's fp32 bar for the tail (tests/test_convtail_gpu.py), per element here: it covers
                 __expf and the hardware reciprocal of mode 4's sigmoid
"""
import numpy as np
import torch

from oracle import convtail as oc

F64 = torch.float64
U = 2.0 ** -24
RHO = {torch.bfloat16: 2.0 ** -8, torch.float32: 0.0}
INTRINSIC = 2e-5
_TINY = 1e-300


def c_float(v):
    """The value a C ``float`` argument holds (eps and momentum cross the C ABI as floats)."""
    return float(np.float32(v))


def ulp32(v):
    """Spacing of fp32 at |fp32(v)|, as float64."""
    r = v.to(F64).abs().to(torch.float32)
    return (torch.nextafter(r, torch.full_like(r, torch.inf)) - r).to(F64)


def finite(*tensors):
    return all(t is None or bool(torch.isfinite(t.to(F64)).all()) for t in tensors)


def ratio(err, bound):
    """max(err / bound); infinite when either holds a NaN or an infinity (inputs are finite: so must the outputs be)."""
    if not err.numel():
        return 0.0
    if not finite(err, bound):
        return float("inf")
    return float((err / (bound + _TINY)).max())


def mismatch(got, want):
    """0.0 when ``got`` (the kernel's dtype) holds exactly the values of ``want`` (float64, representable in that
    dtype) bit for bit, the sign of zero included, else 1 + the number of elements that differ; infinite when the
    shapes differ or either side is not finite (a NaN that the replay reproduces from a NaN coefficient is no
    agreement)."""
    if got.shape != want.shape or not finite(got, want):
        return float("inf")
    want = want.to(got.dtype)
    bits = torch.int16 if got.dtype == torch.bfloat16 else torch.int32
    n = int((got.contiguous().view(bits) != want.contiguous().view(bits)).sum())
    return 0.0 if n == 0 else 1.0 + n


# ------------------------------------------------------------------------------------------------- statistics

def check_stats(x, weight, bias, eps, momentum, rm0, rv0, training, mean_invstd, scale_shift, rm, rv, exact):
    """Coefficients and running statistics against oracle.convtail.tail_stats.

    exact=True -- for inputs on which every fp32 partial sum of (x - x0) and (x - x0)^2 is exact in any order
    (integers with |x - x0| <= 16 and rows < 65536; rows <= 2; eval mode): the kernel combines exact sums in double,
    so ``mean`` is fp32(float64 mean) bit for bit; ``invstd``, ``a`` and the running statistics are within 1 fp32 ulp;
    ``b`` = bias - mean a is within 2^-22 (|bias| + |mean a|) (mean 2^-24, a 2^-23, the fused multiply-add 2^-24).
    Eval mode: mean is running_mean itself and the buffers come back bit-identical.

    exact=False -- any input, gross errors only: fp32 sums of d = x - x0 over `rows` terms,
        |mean - ref|  <=  u |ref| + rows u mean|d|
        |var  - ref|  <=  2u (var + eps) + (rows + 1) u mean(d^2) + 2 |mean(d)| rows u mean|d|
    with var recovered from the returned invstd (hence the 2u (var + eps)); the running statistics inherit these
    scaled by the momentum, plus their own rounding; ``a`` and ``b`` must follow from the kernel's own mean and
    invstd (a is w times the unrounded invstd, rounded once: within 1 ulp plus |w| times half an ulp of the returned
    invstd; b within 2u (|bias| + |mean a|))."""
    x64 = x.to(F64)
    rows = x64.shape[0]
    eps, momentum = c_float(eps), c_float(momentum)
    ref = oc.tail_stats(x64, weight, bias, eps, rm0, rv0, momentum, training)
    mean_k, invstd_k = mean_invstd[0].to(F64), mean_invstd[1].to(F64)
    a_k, b_k = scale_shift[0].to(F64), scale_shift[1].to(F64)
    w64 = torch.ones_like(a_k) if weight is None else weight.to(F64)
    bias64 = torch.zeros_like(a_k) if bias is None else bias.to(F64)
    out = {"finite": 0.0 if finite(mean_invstd, scale_shift, rm, rv) else float("inf")}
    if exact:
        out["mean"] = mismatch(mean_invstd[0], ref["mean"].to(torch.float32).to(F64))
        out["invstd"] = ratio((invstd_k - ref["invstd"]).abs(), ulp32(ref["invstd"]))
        out["a"] = ratio((a_k - ref["a"]).abs(), ulp32(ref["a"]))
        out["b"] = ratio((b_k - ref["b"]).abs(), 2.0 ** -22 * (bias64.abs() + (ref["mean"] * ref["a"]).abs()))
        if rm is not None:
            if training:
                out["running_mean"] = ratio((rm.to(F64) - ref["running_mean"]).abs(), ulp32(ref["running_mean"]))
                out["running_var"] = ratio((rv.to(F64) - ref["running_var"]).abs(), ulp32(ref["running_var"]))
            else:
                out["running_mean"], out["running_var"] = mismatch(rm, rm0.to(F64)), mismatch(rv, rv0.to(F64))
        return out
    assert training, "the loose statistics check is for training mode"
    d = x64 - x64[0]
    m1, abs1, m2 = d.mean(0), d.abs().mean(0), (d * d).mean(0)
    mean_bound = U * ref["mean"].abs() + rows * U * abs1
    var_bound = 2 * U * (ref["var"] + eps) + (rows + 1) * U * m2 + 2 * m1.abs() * rows * U * abs1
    out["mean"] = ratio((mean_k - ref["mean"]).abs(), mean_bound)
    out["var"] = ratio((invstd_k ** -2 - eps - ref["var"]).abs(), var_bound)
    out["a"] = ratio((a_k - w64 * invstd_k).abs(), ulp32(w64 * invstd_k) + 0.5 * w64.abs() * ulp32(invstd_k))
    out["b"] = ratio((b_k - (bias64 - mean_k * a_k)).abs(), 2 * U * (bias64.abs() + (mean_k * a_k).abs()))
    if rm is not None:
        unb = rows / (rows - 1.0) if rows > 1 else 1.0
        out["running_mean"] = ratio((rm.to(F64) - ref["running_mean"]).abs(),
                                    ulp32(ref["running_mean"]) + momentum * mean_bound)
        out["running_var"] = ratio((rv.to(F64) - ref["running_var"]).abs(),
                                   ulp32(ref["running_var"]) + momentum * unb * var_bound)
    return out


# ------------------------------------------------------------------------------------------------- forward

def check_forward(x, res, scale_shift, mode, y):
    """y against the replay from the kernel's own ``scale_shift``.  Modes 1 / 2 / 3: bit-equal on every element.
    Mode 4: |y - silu64(z_r)| <= rho |ref| + 2e-5 max(1, |ref|), z_r the exactly replayed rounded pre-activation.
    -> ({"y": ratio}, the replay, for check_backward)."""
    dtype = y.dtype
    if not finite(scale_shift, y):                       # nothing to replay from / a NaN or infinity in the output
        return {"y": float("inf")}, None
    fwd = oc.tail_forward_replay(x.to(F64), None if res is None else res.to(F64), scale_shift[0], scale_shift[1],
                                 mode, dtype)
    if fwd["y"].shape != y.shape:
        return {"y": float("inf")}, fwd
    if mode != 4:
        return {"y": mismatch(y, fwd["y"])}, fwd
    ref = fwd["y"]
    bound = RHO[dtype] * ref.abs() + INTRINSIC * ref.abs().clamp_min(1.0)
    return {"y": ratio((y.to(F64) - ref).abs(), bound)}, fwd


# ------------------------------------------------------------------------------------------------- backward

def check_backward(x, res, dy, mean_invstd, scale_shift, mode, dx, dweight, dbias, dres, integer_dy, fwd=None):
    """Gradients against the replay of the routing, every element.

    dbias, dweight (n = rows):
      integer_dy (modes 1 / 2 / 3, dy integer-valued with rows * max|dy| < 2^24): every partial sum of dz is exact,
      so dbias is fp32(float64 sum) bit for bit; otherwise |dbias - ref| <= (n + 4) u sum|dz|.
      |dweight - ref| <= (n + 4) u sum|dz xhat|   (x - mean, n - 1 fused accumulations, times invstd, one store).
      Mode 4 adds 2e-5 times the same magnitude sums for silu'.
    dx, from the kernel's own a, mean, invstd, dweight, dbias:  ref = a dz + p + q x,
      |dx - ref| <= rho |ref| + 2^-21 (|a dz| + |a dbias / n| + |q| (|x| + |mean|))   [+ 2e-5 |a dy| in mode 4]
      (roundings of p, q, the two fused multiply-adds: at most 3 u on each term).
    dres: bit-equal to the routed dy."""
    dtype = dx.dtype
    x64, dy64 = x.to(F64), dy.to(F64)
    n = x64.shape[0]
    mean_k, invstd_k, a_k = mean_invstd[0].to(F64), mean_invstd[1].to(F64), scale_shift[0].to(F64)
    if not finite(mean_invstd, scale_shift):
        return {"dbias": float("inf"), "dweight": float("inf"), "dx": float("inf")}
    if fwd is None:
        fwd = oc.tail_forward_replay(x64, None if res is None else res.to(F64), scale_shift[0], scale_shift[1], mode,
                                     dtype)
    rep = oc.tail_backward_replay(x64, dy64, fwd, mode, mean_k, invstd_k, dweight, dbias, a_k, n)
    extra = INTRINSIC if mode == 4 else 0.0
    out = {}
    if integer_dy:
        assert mode != 4
        out["dbias"] = mismatch(dbias, rep["sum_dz"].to(torch.float32).to(F64))
    else:
        out["dbias"] = ratio((dbias.to(F64) - rep["sum_dz"]).abs(), ((n + 4) * U + extra) * rep["mag_dz"])
    out["dweight"] = ratio((dweight.to(F64) - rep["sum_dzx"]).abs(), ((n + 4) * U + extra) * rep["mag_dzx"])
    if dx.shape != x.shape:
        out["dx"] = float("inf")
        return out
    ref = rep["dx"]
    bound = RHO[dtype] * ref.abs() + 2.0 ** -21 * ((a_k * rep["dz"]).abs() + (a_k * dbias.to(F64) / n).abs() +
                                                  rep["q"].abs() * (x64.abs() + mean_k.abs()))
    if mode == 4:
        bound = bound + INTRINSIC * (a_k * dy64).abs()
    out["dx"] = ratio((dx.to(F64) - ref).abs(), bound)
    if mode == 3:
        out["dres"] = mismatch(dres, rep["dres"])
    return out


# ------------------------------------------------------------------------------------------------- cases

def make_case(mode, dtype, rows=74, c=16, integer=True, seed=0, wide_bias=False, offset=0.0):
    """Inputs of one tail call as CPU tensors, activations [rows, C] in ``dtype``.
    integer: x in {-8..8} plus a per-channel integer offset in [-100, 100] (exact in bf16; exact statistics; frequent
    ties); else Gaussian with per-channel scale and shift.  dy is integer-valued in {-4..4} for modes 1 / 2 / 3 (exact
    sums), Gaussian for mode 4.  wide_bias: z around 8 with slope 0.5, so that neighbouring bf16 x collapse onto one
    bf16 z and ties of the ROUNDED pre-activation are frequent."""
    g = torch.Generator().manual_seed(1000 * mode + seed)
    if integer:
        x = (torch.randint(-8, 9, (rows, c), generator=g) + torch.randint(-100, 101, (c,), generator=g)).to(dtype)
    else:
        x = (torch.randn(rows, c, generator=g) * (torch.rand(c, generator=g) * 3 + 0.2) +
             torch.randn(c, generator=g) * 2 + offset).to(dtype)
    res = torch.randn(rows, c, generator=g).to(dtype) if mode == 3 else None
    out_rows = rows // 2 if mode == 2 else rows
    dy = torch.randn(out_rows, c, generator=g).to(dtype) if mode == 4 else \
        torch.randint(-4, 5, (out_rows, c), generator=g).to(dtype)
    weight = torch.rand(c, generator=g) + 0.5
    bias = torch.randn(c, generator=g) * 0.3
    if wide_bias:
        weight, bias = torch.full((c,), 0.5), torch.full((c,), 8.0)
    return dict(x=x, res=res, dy=dy, weight=weight, bias=bias, rm0=torch.randn(c, generator=g),
                rv0=torch.rand(c, generator=g) + 0.5, eps=1e-5, momentum=0.1)


def run_checks(case, out, mode, exact_stats, training=True, backward=True):
    """Every check on one set of outputs (dict: y, mean_invstd, scale_shift, running_mean, running_var and, with
    ``backward``, dx, dweight, dbias, dres) -> {"stats.mean": ratio, "forward.y": ..., "backward.dx": ..., ...}."""
    x, res, dy = case["x"], case["res"], case["dy"]
    ratios = {}
    st = check_stats(x, case["weight"], case["bias"], case["eps"], case["momentum"], case["rm0"], case["rv0"], training,
                     out["mean_invstd"], out["scale_shift"], out["running_mean"], out["running_var"], exact=exact_stats)
    ratios.update({"stats." + k: v for k, v in st.items()})
    fw, fwd = check_forward(x, res, out["scale_shift"], mode, out["y"])
    ratios.update({"forward." + k: v for k, v in fw.items()})
    if backward:
        bw = check_backward(x, res, dy, out["mean_invstd"], out["scale_shift"], mode, out["dx"], out["dweight"],
                            out["dbias"], out["dres"], integer_dy=mode != 4, fwd=fwd)
        ratios.update({"backward." + k: v for k, v in bw.items()})
    return ratios


# ------------------------------------------------------------------------------------------------- depthwise conv

def dw_output_ratio(got, ref, mag, k):
    """Forward / data gradient: |err| <= rho |ref| + 2 K u S, S the magnitude sum (K fused accumulations)."""
    if got.shape != ref.shape:
        return float("inf")
    return ratio((got.to(F64) - ref).abs(), RHO[got.dtype] * ref.abs() + 2 * k * U * mag)


def dw_grad_ratio(got, ref, mag, b, t):
    """dweight / dbias (fp32): |err| <= (B T + 4) u S."""
    if got.shape != ref.shape:
        return float("inf")
    return ratio((got.to(F64) - ref).abs(), (b * t + 4) * U * mag)


def worst(ratios):
    """The largest ratio; infinite if any is a NaN (Python's max would drop it)."""
    return max((v if v == v else float("inf") for v in ratios.values()), default=0.0)


def passes(ratios):
    return all(v <= 1.0 for v in ratios.values())


def fmt(ratios):
    return ", ".join(f"{k} {v:.3g}" for k, v in ratios.items())
