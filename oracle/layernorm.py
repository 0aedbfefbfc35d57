"""Float64 oracle and exact replay of the fused LayerNorm [-> ReLU] (csrc/layernorm.hip) -- CPU only, torch.

Three layers:

  * ``plain`` -- LayerNorm [-> ReLU] over the last dimension and its three gradients in float64, no rounding anywhere
    (pinned against ``torch.nn.functional.layer_norm`` + autograd by tests/test_layernorm_oracle_cpu.py).
  * ``row_stats_replay`` / ``forward_replay`` -- the forward kernel restated with its rounding points.  One wavefront
    owns a row; element (chunk c, lane l, j) is column (c * 64 + l) * V + j; a lane adds its kChunks * V values in
    (c, j) order, the 64 lane sums go through the xor butterfly 32, 16, .., 1, and every other operation is a single
    fp32 subtraction, multiplication or an explicit ``fmaf``.  ``fmaf_exact`` / ``add_exact`` (oracle/convtail.py)
    are those operations computed in float64, so the replay is exact to the bit -- except ``rsqrtf``, whose result
    the kernel returns and the replay takes as given.
  * ``backward_replay`` -- ``xhat`` and the ReLU mask as the backward kernel recomputes them, the column sums
    d(weight), d(bias) in the kernel's order (``wave_sums`` -> ``block_fold`` -> ``final_sum``), and dx in float64 from
    the same xhat, mask and statistics (its fp32 grouping is the compiler's: bounded by the checks, not replayed).

All activations are ``[rows, D]`` float64 tensors whose values are representable in the activation dtype; weight and
bias ``[D]`` and the statistics ``[rows]`` hold fp32 values.
"""
import torch

from oracle.convtail import F64, _rounder, add_exact, fmaf_exact, round_bf16  # noqa: F401  (round_bf16: re-exported)

WAVES = 4                 # wavefronts (rows in flight) per block
MAX_BLOCKS = 512          # backward: partial rows of the column sums
FINAL_GROUPS = 16         # final kernel: row groups per column
GEOMETRY = {256: (4, 1), 512: (8, 1), 1024: (8, 2), 2048: (8, 4)}        # D -> (V, kChunks), the dispatch switch

_XOR = (32, 16, 8, 4, 2, 1)


def geometry(d):
    if d not in GEOMETRY:
        raise ValueError(f"unsupported width {d}")
    return GEOMETRY[d]


def backward_blocks(rows):
    return min((rows + WAVES - 1) // WAVES, MAX_BLOCKS)


def sum_depth(d):
    """Additions on the longest path from an element to the row sum: kChunks * V in the lane, 6 in the butterfly."""
    v, k = geometry(d)
    return v * k + 6


def column_depth(rows, rows_per_launch=None):
    """Additions on the longest path from a row's term to a column sum: the wavefront's rows, 3 in the block fold, 5 in
    the final kernel's halving tree, 16 over its groups."""
    nw = WAVES * backward_blocks(rows) if rows_per_launch is None else rows_per_launch
    return (rows + nw - 1) // nw + (WAVES - 1) + 5 + FINAL_GROUPS


def c_float(v):
    """The value a C ``float`` argument holds (eps crosses the C ABI as a float)."""
    return float(torch.tensor(v, dtype=torch.float32))


def round_f32(v):
    """fp32 RNE of float64 values that are EXACT results (a product of two fp32 numbers, a power-of-two scaling)."""
    return v.to(torch.float32).to(F64)


def lanes(t, d):
    """[rows, D] -> [rows, kChunks, 64, V]: [r, c, l, j] is column (c * 64 + l) * V + j."""
    v, k = geometry(d)
    return t.reshape(t.shape[0], k, 64, v)


def wave_sum(s):
    """The xor butterfly over the 64 lane values s [rows, 64]: every lane ends with the same bits (fp32 addition
    commutes), returned [rows]."""
    idx = torch.arange(64)
    for m in _XOR:
        s = add_exact(s, s[:, idx ^ m])
    return s[:, 0]


def row_mean_replay(x, d):
    """The fp32 row mean: lane chains in (c, j) order from +0, butterfly, times the exact 1 / D."""
    v, k = geometry(d)
    xl = lanes(x.to(F64), d)
    s = torch.zeros(x.shape[0], 64, dtype=F64)
    for c in range(k):
        for j in range(v):
            s = add_exact(s, xl[:, c, :, j])
    return round_f32(wave_sum(s) / d)


def row_var_replay(x, mean, d):
    """The fp32 biased variance about the given fp32 mean: q = fmaf(dev, dev, q) on dev = fp32(x - mean) in the same
    order, butterfly, times 1 / D."""
    v, k = geometry(d)
    xl = lanes(x.to(F64), d)
    q = torch.zeros(x.shape[0], 64, dtype=F64)
    for c in range(k):
        for j in range(v):
            dev = add_exact(xl[:, c, :, j], -mean[:, None])
            q = fmaf_exact(dev, dev, q)
    return round_f32(wave_sum(q) / d)


def row_stats_replay(x, eps, d):
    """-> (mean [rows], var + eps [rows]): the fp32 mean the kernel stores and the fp32 argument of its ``rsqrtf``."""
    mean = row_mean_replay(x, d)
    return mean, add_exact(row_var_replay(x, mean, d), torch.tensor(c_float(eps), dtype=F64))


def xhat_replay(x, mean, rstd):
    """fp32((fp32(x - mean)) * rstd): the product of two fp32 numbers is exact in float64, one rounding."""
    return round_f32(add_exact(x.to(F64), -mean.to(F64)[:, None]) * rstd.to(F64)[:, None])


def forward_replay(x, weight, bias, mean, rstd, relu, dtype):
    """y from GIVEN fp32 statistics: z = fmaf(xhat, w, b); fmaxf(z, 0) with ``relu`` (+0 where z <= 0, the sign of a
    zero included); store rounding of ``dtype``.  dtype float64: no rounding anywhere.
    -> dict(y, z, xhat)."""
    x, w, b, mean, rstd = (t.to(F64) for t in (x, weight, bias, mean, rstd))
    if dtype == F64:
        xh = (x - mean[:, None]) * rstd[:, None]
        z = xh * w + b
    else:
        xh = xhat_replay(x, mean, rstd)
        z = fmaf_exact(xh, w, b)
    y = torch.where(z > 0, z, torch.zeros((), dtype=F64)) if relu else z
    return dict(y=_rounder(dtype)(y), z=z, xhat=xh)


def wave_sums(g, xh, rows_per_launch):
    """The running column sums of every wavefront of the grid, [rows_per_launch, D] each: wavefront i walks rows
    i, i + rows_per_launch, ... with dw = fmaf(g, xhat, dw) and db += g from +0."""
    rows, d = g.shape
    dw = torch.zeros(rows_per_launch, d, dtype=F64)
    db = torch.zeros(rows_per_launch, d, dtype=F64)
    for lo in range(0, rows, rows_per_launch):
        n = min(rows, lo + rows_per_launch) - lo
        dw[:n] = fmaf_exact(g[lo:lo + n], xh[lo:lo + n], dw[:n])
        db[:n] = add_exact(db[:n], g[lo:lo + n])
    return dw, db


def block_fold(w):
    """[blocks * 4, D] -> [blocks, D]: wavefronts 1, 2, 3 added onto wavefront 0, in that order."""
    w = w.view(-1, WAVES, w.shape[-1])
    acc = w[:, 0]
    for k in range(1, WAVES):
        acc = add_exact(acc, w[:, k])
    return acc


def final_sum(partial):
    """[blocks <= 512, D] -> [D]: thread (group, column) holds rows group + 16 k (k < 32, absent rows +0), folds them
    with the halving tree v[k] += v[k + width], width = 16, 8, .., 1; then the 16 groups are added in order from +0."""
    blocks, d = partial.shape
    per = MAX_BLOCKS // FINAL_GROUPS
    v = torch.zeros(MAX_BLOCKS, d, dtype=F64)
    v[:blocks] = partial
    v = v.view(per, FINAL_GROUPS, d)
    width = per // 2
    while width >= 1:
        v = add_exact(v[:width], v[width:2 * width])
        width //= 2
    total = torch.zeros(d, dtype=F64)
    for grp in range(FINAL_GROUPS):
        total = add_exact(total, v[0, grp])
    return total


def backward_replay(x, dy, weight, bias, mean, rstd, relu, dtype, rows_per_launch=None, mask=None):
    """The backward kernel from GIVEN fp32 statistics.  ``xhat`` as in the forward; the mask is
    ``fmaf(xhat, w, b) > 0`` recomputed (``mask``: use this one instead, e.g. y > 0 of a forward output); g = dy where
    the mask holds, +0 elsewhere.  dweight / dbias in the kernel's order; ``rows_per_launch`` = rows one sweep of the
    grid covers, 4 * min(ceil(rows / 4), 512) unless given.  dx in float64:

        dx = rstd (g w - mean(g w) - xhat mean(g w xhat))

    -> dict(dx, dweight, dbias, xhat, mask, g, partial_dweight, partial_dbias)."""
    assert dtype in (torch.float32, torch.bfloat16)
    x, dy, w, b, mean, rstd = (t.to(F64) for t in (x, dy, weight, bias, mean, rstd))
    rows = x.shape[0]
    nw = WAVES * backward_blocks(rows) if rows_per_launch is None else rows_per_launch
    assert nw % WAVES == 0 and nw // WAVES <= MAX_BLOCKS
    xh = xhat_replay(x, mean, rstd)
    if mask is None:
        mask = fmaf_exact(xh, w, b) > 0 if relu else torch.ones_like(x, dtype=torch.bool)
    g = torch.where(mask, dy, torch.zeros((), dtype=F64))
    dw_w, db_w = wave_sums(g, xh, nw)
    pw, pb = block_fold(dw_w), block_fold(db_w)
    gw = g * w
    c1, c2 = gw.mean(1, keepdim=True), (gw * xh).mean(1, keepdim=True)
    dx = rstd[:, None] * (gw - c1 - xh * c2)
    return dict(dx=dx, dweight=final_sum(pw), dbias=final_sum(pb), xhat=xh, mask=mask, g=g, partial_dweight=pw,
                partial_dbias=pb)


def plain(x, weight, bias, eps, relu, dy=None):
    """LayerNorm [-> ReLU] and its gradients in float64, two-pass biased variance, nothing rounded.
    -> dict(y, z, mean, var, rstd[, dx, dweight, dbias])."""
    x, w, b = x.to(F64), weight.to(F64), bias.to(F64)
    mean = x.mean(1)
    var = ((x - mean[:, None]) ** 2).mean(1)
    rstd = 1.0 / torch.sqrt(var + eps)
    xh = (x - mean[:, None]) * rstd[:, None]
    z = xh * w + b
    out = dict(y=torch.relu(z) if relu else z, z=z, mean=mean, var=var, rstd=rstd)
    if dy is not None:
        g = dy.to(F64) * (z > 0) if relu else dy.to(F64)
        gw = g * w
        c1, c2 = gw.mean(1, keepdim=True), (gw * xh).mean(1, keepdim=True)
        out.update(dx=rstd[:, None] * (gw - c1 - xh * c2), dweight=(g * xh).sum(0), dbias=g.sum(0))
    return out
