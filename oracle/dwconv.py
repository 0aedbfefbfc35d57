"""Float64 restatement of the depthwise Conv1d over time in the channels-last layout of csrc/dwconv.hip -- CPU only.

    y[b, t, d] = bias[d] + sum_k w[d, k] x[b, t + k - pad, d],      pad = (K - 1) / 2,  zero outside 0 <= t < T

which is nn.Conv1d(D, D, K, padding=pad, groups=D) of model_conformer.py:71-96 on [B, D, T], transposed.  Every
function returns (value, magnitude): the magnitude is the same expression on absolute values, the scale of a
worst-case accumulation bound.  x, dy: [B, T, D]; w: [D, K]; bias: [D] or None.  All float64.
"""
import torch
import torch.nn.functional as F

F64 = torch.float64


def _taps(x, k):
    """[B, T, D] -> [K, B, T, D]: slice k holds x[b, t + k - pad, d] (zero outside the sequence)."""
    pad = (k - 1) // 2
    t = x.shape[1]
    xp = F.pad(x.to(F64), (0, 0, pad, pad))
    return torch.stack([xp[:, i:i + t] for i in range(k)])


def forward(x, w, bias):
    w = w.to(F64)
    win = _taps(x, w.shape[1])                              # [K, B, T, D]
    wk = w.t()[:, None, None, :]                            # [K, 1, 1, D]
    y, mag = (win * wk).sum(0), (win.abs() * wk.abs()).sum(0)
    if bias is not None:
        y, mag = y + bias.to(F64), mag + bias.to(F64).abs()
    return y, mag


def dgrad(dy, w):
    """dx[b, t, d] = sum_k w[d, K - 1 - k] dy[b, t + k - pad, d]: the forward with the taps flipped, no bias."""
    return forward(dy, w.to(F64).flip(1), None)


def wgrad(x, dy, k):
    """dweight[d, k] = sum_{b, t} dy[b, t, d] x[b, t + k - pad, d];  dbias[d] = sum_{b, t} dy[b, t, d].
    -> (dweight, mag_dweight, dbias, mag_dbias)."""
    dy = dy.to(F64)
    win = _taps(x, k)
    dw = (win * dy).sum((1, 2)).t()
    mag = (win.abs() * dy.abs()).sum((1, 2)).t()
    return dw, mag, dy.sum((0, 1)), dy.abs().sum((0, 1))
