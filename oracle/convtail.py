"""Float64 oracle and exact replay of the fused BatchNorm tails (csrc/convtail.hip) -- CPU only, torch.

Two layers:

  * ``tail_stats`` -- the BatchNorm statistics, coefficients and running-statistics update in float64
    (model_crnn.py:5-17 ``bn``; resnet50_model.py:30-52 ``bn3``; model_conformer.py:71-96 ``batch_norm``).
  * ``tail_forward_replay`` / ``tail_backward_replay`` -- the element-wise stage restated from GIVEN coefficients.
    The kernels return the coefficients they used (``scale_shift``, ``mean_invstd``) and their element-wise stage
    is ``round_T(fmaf(x, a, b))`` followed by comparisons, so with the kernel's own fp32 coefficients the replay is
    exact: ``fmaf_exact`` is the single-rounding fp32 FMA computed in float64, ``round_bf16`` the RNE store
    rounding.  With ``dtype=torch.float64`` every rounding is switched off and the same functions are the plain
    float64 reference of the stock modules (pinned against them by tests/test_tail_oracle_cpu.py).

All activations are ``[rows, C]`` float64 tensors whose values are representable in the activation dtype; the two
rows of a pooling pair are adjacent rows ``(2o, 2o + 1)`` (channels-last ``[B, T, F]`` row order).  Modes follow the
kernels: 1 = BN -> ReLU, 2 = BN -> ReLU -> MaxPool2d((1, 2)), 3 = relu(BN(x) + residual), 4 = silu(BN(x)).
Finite values only.
"""
import torch

F64 = torch.float64


def _two_sum(p, b):
    """Knuth's TwoSum: s = fl(p + b) and e with s + e == p + b exactly."""
    s = p + b
    bb = s - p
    return s, (p - (s - bb)) + (b - bb)


def _round_f32(s, e):
    """fp32 RNE of the exact value s + e (e = the float64 rounding error of s).  The float64 -> fp32 cast of s is
    that value unless s sits exactly on an fp32 rounding midpoint with a non-zero remainder: a midpoint is a
    float64 number, so s and s + e can never lie on different sides of one, and the remainder only decides the
    direction when s IS the midpoint (where the cast alone would tie to even)."""
    r = s.to(torch.float32).to(F64).contiguous()
    flat_r, flat_s, flat_e = r.view(-1), s.reshape(-1), e.reshape(-1)
    idx = torch.nonzero((flat_e != 0) & (flat_r != flat_s) & torch.isfinite(flat_r)).flatten()
    if idx.numel():
        sv, ev, rv = flat_s[idx], flat_e[idx], flat_r[idx]
        toward = torch.where(rv > sv, -torch.inf, torch.inf).to(torch.float32)
        other = torch.nextafter(rv.to(torch.float32), toward).to(F64)      # the fp32 neighbour on the other side of s
        tie = (rv + other) / 2 == sv                                       # adjacent fp32 values: the sum is exact
        pick = torch.where(ev > 0, torch.maximum(rv, other), torch.minimum(rv, other))
        flat_r[idx] = torch.where(tie, pick, rv)
    return r


def fmaf_exact(x, a, b):
    """fp32 ``fmaf(x, a, b)`` (one rounding) for fp32- or bf16-valued float64 inputs, as float64.  The 24 x 24-bit
    product is exact in float64; TwoSum gives the rounding error of adding b."""
    x, a, b = torch.broadcast_tensors(x.to(F64), a.to(F64), b.to(F64))
    return _round_f32(*_two_sum(x * a, b))


def add_exact(u, v):
    """fp32 ``u + v`` for fp32-valued float64 inputs (the residual add of mode 3), as float64."""
    u, v = torch.broadcast_tensors(u.to(F64), v.to(F64))
    return _round_f32(*_two_sum(u, v))


def round_bf16(v):
    """RNE to bfloat16 of fp32-valued data (float32 or float64 tensor) in int32 bit arithmetic; bit-equal to
    ``tensor.bfloat16()`` on finite values.  Returned in v's dtype."""
    bits = v.to(torch.float32).contiguous().view(torch.int32)
    bits = (bits + 0x7FFF + ((bits >> 16) & 1)) & -65536
    return bits.view(torch.float32).to(v.dtype)


def _rounder(dtype):
    if dtype == torch.bfloat16:
        return round_bf16
    if dtype in (torch.float32, torch.float64):
        return lambda v: v
    raise ValueError(f"unsupported activation dtype {dtype}")


def silu(z):
    return z * torch.sigmoid(z)


def silu_grad(z):
    s = torch.sigmoid(z)
    return s * (1 + z * (1 - s))


def tail_stats(x, weight, bias, eps, running_mean, running_var, momentum, training):
    """nn.BatchNorm{1,2}d's statistics on x [rows, C]: biased variance for the normalisation, unbiased (rows > 1)
    for ``running_var``, momentum blend.  Eval mode: coefficients from the running statistics, which stay.
    Everything float64 and unrounded; ``eps`` / ``momentum`` are used as given (the kernels take them as C floats:
    pass ``float(numpy.float32(eps))`` to follow them to the last bit).
    -> dict(mean, var, invstd, a, b, running_mean, running_var)."""
    x = x.to(F64)
    rows, c = x.shape
    weight = torch.ones(c, dtype=F64) if weight is None else weight.to(F64)
    bias = torch.zeros(c, dtype=F64) if bias is None else bias.to(F64)
    rm = None if running_mean is None else running_mean.to(F64)
    rv = None if running_var is None else running_var.to(F64)
    if training:
        mean = x.mean(0)
        var = ((x - mean) ** 2).mean(0)
        if rm is not None:
            unbiased = var * rows / (rows - 1) if rows > 1 else var
            rm = (1.0 - momentum) * rm + momentum * mean
            rv = (1.0 - momentum) * rv + momentum * unbiased
    else:
        mean, var = rm, rv
    invstd = 1.0 / torch.sqrt(var + eps)
    a = weight * invstd
    return dict(mean=mean, var=var, invstd=invstd, a=a, b=bias - mean * a, running_mean=rm, running_var=rv)


def tail_forward_replay(x, residual, a, b, mode, dtype):
    """The element-wise stage from the given coefficients a, b [C]:  z = round_T(fmaf(x, a, b)) -- rounding to the
    activation dtype BEFORE any comparison -- then

      mode 1:  y = relu(z)                                    route 0 where z > 0, else -1
      mode 2:  y = max(relu(z[2o]), relu(z[2o+1]))            route = the larger one, the FIRST on a tie, -1 if y == 0
      mode 3:  t = round_T(z + residual);  y = relu(t)        route 0 where t > 0, else -1
      mode 4:  y = silu(z) in float64 (the kernel's output is this within its intrinsics' error)

    ReLU outputs are +0 where z <= 0.  dtype float64: no rounding anywhere, plain a * x + b.
    -> dict(y, z, route) for modes 1-3 (route: int8, which element of the pair receives dy);
       dict(y, z, dsilu) for mode 4 (z = the rounded pre-activation, dsilu = silu'(z))."""
    x, a, b = x.to(F64), a.to(F64), b.to(F64)
    rnd = _rounder(dtype)
    exact = dtype != torch.float64
    z = rnd(fmaf_exact(x, a, b)) if exact else x * a + b
    zero = torch.zeros((), dtype=F64)
    if mode == 4:
        return dict(y=silu(z), z=z, dsilu=silu_grad(z))
    if mode == 1:
        return dict(y=torch.where(z > 0, z, zero), z=z, route=torch.where(z > 0, 0, -1).to(torch.int8))
    if mode == 3:
        residual = residual.to(F64)
        t = rnd(add_exact(z, residual)) if exact else z + residual
        return dict(y=torch.where(t > 0, t, zero), z=t, route=torch.where(t > 0, 0, -1).to(torch.int8))
    if mode == 2:
        r0 = torch.where(z[0::2] > 0, z[0::2], zero)
        r1 = torch.where(z[1::2] > 0, z[1::2], zero)
        second = r1 > r0
        y = torch.where(second, r1, r0)
        route = torch.where(y > 0, second.to(torch.int8), torch.tensor(-1, dtype=torch.int8))
        return dict(y=y, z=z, route=route)
    raise ValueError(f"mode {mode}")


def tail_backward_replay(x, dy, fwd, mode, mean, invstd, dweight=None, dbias=None, a=None, n=None):
    """Backward of the tail from the routing (``fwd`` = tail_forward_replay's result) in float64:

      dz    = dy scattered to the routed element (modes 1-3) or dy * silu'(z) (mode 4), on x's [rows, C]
      sum_dz, sum_dzx   = per-channel sums of dz and dz * xhat,  xhat = (x - mean) * invstd
      mag_dz, mag_dzx   = the same sums of absolute values

    and, given the parameter gradients and the scale a (the kernel's own, or the sums above),

      dx   = a dz + p + q x,   q = -a (dweight / n) invstd,   p = -a dbias / n - q mean      (n = rows)
      dres = dz  (mode 3: the routed dy)

    -> dict(dz, sum_dz, sum_dzx, mag_dz, mag_dzx[, dx, p, q, dres])."""
    x, dy, mean, invstd = x.to(F64), dy.to(F64), mean.to(F64), invstd.to(F64)
    if mode == 4:
        dz = dy * fwd["dsilu"]
    elif mode == 2:
        dz = torch.zeros_like(x)
        dz[0::2] = torch.where(fwd["route"] == 0, dy, 0.0)
        dz[1::2] = torch.where(fwd["route"] == 1, dy, 0.0)
    else:
        dz = torch.where(fwd["route"] == 0, dy, 0.0)
    t = dz * ((x - mean) * invstd)
    out = dict(dz=dz, sum_dz=dz.sum(0), sum_dzx=t.sum(0), mag_dz=dz.abs().sum(0), mag_dzx=t.abs().sum(0))
    if dweight is not None:
        a, n = a.to(F64), float(x.shape[0] if n is None else n)
        q = -a * (dweight.to(F64) / n) * invstd
        p = -a * dbias.to(F64) / n - q * mean
        out.update(dx=a * dz + p + q * x, p=p, q=q)
        if mode == 3:
            out["dres"] = dz
    return out
