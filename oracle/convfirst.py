"""Float64 oracle and exact replay of the first encoder block (csrc/convfirst.hip) -- CPU only, torch.

  Conv3x3(4 -> 64, pad 1, no bias) -> BatchNorm2d (training) -> ReLU -> MaxPool2d((1, 2))          (model_crnn.py:5-17)

The kernels recompute x1 = round_bf16(conv) wherever they need it and never store it.  On inputs whose 36-term fp32
accumulation is exact in any order (every partial sum representable in fp32: tests/convfirst_checks.py builds two such
families) x1 is the float64 convolution rounded once, bit for bit, and everything after it is the BN -> ReLU -> pool
tail of oracle/convtail.py (mode 2) on x1:

  * ``x1``       -- the convolution as [B T F, 64] rows in channels-last order (a pooling pair = adjacent rows);
  * ``stats``    -- convfirst_stats_final_kernel restated: unshifted sums, var = E[x^2] - E[x]^2 clamped at 0, the fp32
                    invstd, a = fl32(weight * invstd_f32), b = bias - mean_f32 * a;
  * ``backward`` -- the routing of ``tail_forward_replay(mode 2)``, the sums and p, q of convfirst_bwd_final_kernel,
                    dx1 = round_bf16(fmaf(a, dz, fmaf(q, x, p))) and the weight gradient dW = dx1^T im2col(x) with its
                    magnitude sum S = |dx1|^T |im2col(x)|, both float64.

With ``dtype=torch.float64`` every rounding is switched off and the same functions are the plain float64 block
(pinned to the stock modules and their autograd by tests/test_convfirst_oracle_cpu.py).  Finite values only.
"""
import torch
import torch.nn.functional as F

from oracle.convtail import F64, fmaf_exact, round_bf16, tail_forward_replay

COUT, CIN, K = 64, 4, 36


def f32(v):
    """fp32 RNE of a float64 tensor, as float64."""
    return v.to(torch.float32).to(F64)


def conv(x, w):
    """float64 conv2d(padding=1) of x [B, 4, T, F] with w [64, 4, 3, 3] -> [B T F, 64] rows, channels-last order."""
    v = F.conv2d(x.to(F64), w.to(F64), padding=1)
    return v.permute(0, 2, 3, 1).reshape(-1, v.shape[1]).contiguous()


def x1(x, w, dtype=torch.bfloat16):
    """The block's convolution output as the kernels form it: the float64 convolution of the bf16 values, rounded once
    to bf16.  This IS the kernel's x1 whenever the exact convolution is representable in fp32 (``round_bf16`` casts to
    fp32 first, which is then no rounding); dtype float64: unrounded."""
    v = conv(x, w)
    return round_bf16(v) if dtype == torch.bfloat16 else v


def im2col(x):
    """[B, 4, T, F] -> [B T F, 36] float64, zero padded; column ci * 9 + r * 3 + s, as w.reshape(64, 36)."""
    b, c, t, f = x.shape
    cols = F.unfold(x.to(F64), kernel_size=3, padding=1)                      # [B, 36, T F]
    return cols.transpose(1, 2).reshape(b * t * f, c * 9).contiguous()


def finalise(s1, s2, n, weight, bias, eps, rm0, rv0, momentum, dtype=torch.bfloat16):
    """convfirst_stats_final_kernel from the per-channel sums s1 = sum x, s2 = sum x^2 (float64) over n rows.
    -> dict(mean, var, invstd, a, b, b_unfused, running_mean, running_var), float64 tensors.  With rounding (dtype
    bf16) mean / invstd / a / b hold the fp32 values the kernel stores: b is the fused bias - mean a (one rounding),
    b_unfused the same with the product rounded first -- the compiler may emit either.  The running statistics are
    left unrounded (the kernel's are their fp32 rounding)."""
    n = float(n)
    weight, bias, rm0, rv0 = weight.to(F64), bias.to(F64), rm0.to(F64), rv0.to(F64)
    mean = s1 / n
    var = (s2 / n - mean * mean).clamp_min(0.0)
    unbiased = var * n / (n - 1.0) if n > 1 else var
    rm = (1.0 - momentum) * rm0 + momentum * mean
    rv = (1.0 - momentum) * rv0 + momentum * unbiased
    invstd = 1.0 / torch.sqrt(var + eps)
    if dtype == torch.float64:
        a = weight * invstd
        b = bias - mean * a
        return dict(mean=mean, var=var, invstd=invstd, a=a, b=b, b_unfused=b, running_mean=rm, running_var=rv)
    mean_f, invstd_f = f32(mean), f32(invstd)
    a = f32(weight * invstd_f)
    return dict(mean=mean_f, var=var, invstd=invstd_f, a=a, b=fmaf_exact(-mean_f, a, bias),
                b_unfused=f32(bias - f32(mean_f * a)), running_mean=rm, running_var=rv)


def stats(x1_rows, weight, bias, eps, rm0, rv0, momentum, dtype=torch.bfloat16):
    """The BatchNorm statistics and coefficients of x1 [rows, 64] the way the kernels form them (``finalise``)."""
    v = x1_rows.to(F64)
    return finalise(v.sum(0), (v * v).sum(0), v.shape[0], weight, bias, eps, rm0, rv0, momentum, dtype)


def route(x1_rows, dy, a, b, dtype=torch.bfloat16, fwd=None):
    """dz [rows, 64]: dy [rows / 2, 64] scattered to the bin that won the pooling (the first on a tie), nothing where
    the pooled output is 0.  ``fwd``: the forward replay from the same a, b, if the caller has it.
    -> (dz, the forward replay)."""
    if fwd is None:
        fwd = tail_forward_replay(x1_rows, None, a, b, 2, dtype)
    dy = dy.to(F64)
    dz = torch.zeros_like(fwd["z"])
    dz[0::2] = torch.where(fwd["route"] == 0, dy, 0.0)
    dz[1::2] = torch.where(fwd["route"] == 1, dy, 0.0)
    return dz, fwd


def bwd_final(s_dz, s_dzx_raw, n, a, mean, invstd, dtype=torch.bfloat16):
    """convfirst_bwd_final_kernel from s_dz = sum dz and s_dzx_raw = sum dz x (float64):
    sum dz xhat = (s_dzx_raw - mean s_dz) invstd,  q = -a (s_dzx / n) invstd,  p = -a (s_dz / n) - q mean,
    with dgamma, dbeta, p, q rounded to fp32 unless dtype is float64."""
    n = float(n)
    a, mean, invstd = a.to(F64), mean.to(F64), invstd.to(F64)
    s_dzx = (s_dzx_raw - mean * s_dz) * invstd
    q = -a * (s_dzx / n) * invstd
    p = -a * (s_dz / n) - q * mean
    rnd = (lambda v: v) if dtype == torch.float64 else f32
    return dict(s_dz=s_dz, s_dzx=s_dzx, dbeta=rnd(s_dz), dgamma=rnd(s_dzx), p=rnd(p), q=rnd(q))


def dx1_of(x1_rows, dz, a, p, q, dtype=torch.bfloat16):
    """-> (dx1, pre): dx1 = round_bf16(pre), pre = fmaf(a, dz, fmaf(q, x, p)) in fp32; float64: a dz + q x + p."""
    x = x1_rows.to(F64)
    if dtype == torch.float64:
        pre = a * dz + q * x + p
        return pre, pre
    pre = fmaf_exact(a, dz, fmaf_exact(q, x, p))
    return round_bf16(pre), pre


def backward(x1_rows, cols, dy, a, b, mean, invstd, dtype=torch.bfloat16, fwd=None):
    """The block's backward from x1 [rows, 64], cols = im2col(x) [rows, 36], dy [rows / 2, 64] and the forward's
    coefficients a, b, mean, invstd [64].
    -> dict(fwd, dz, s_dz, s_dzx, mag_dzx, dbeta, dgamma, p, q, dx1, pre, dW [64, 4, 3, 3], S [64, 4, 3, 3])."""
    x = x1_rows.to(F64)
    a, b, mean, invstd = a.to(F64), b.to(F64), mean.to(F64), invstd.to(F64)
    dz, fwd = route(x, dy, a, b, dtype, fwd)
    out = bwd_final(dz.sum(0), (dz * x).sum(0), x.shape[0], a, mean, invstd, dtype)
    dx1, pre = dx1_of(x, dz, a, out["p"], out["q"], dtype)
    out.update(fwd=fwd, dz=dz, mag_dzx=(dz * ((x - mean) * invstd)).abs().sum(0), dx1=dx1, pre=pre,
               dW=(dx1.t() @ cols).view(COUT, CIN, 3, 3), S=(dx1.abs().t() @ cols.abs()).view(COUT, CIN, 3, 3))
    return out
