"""numpy float64 restatement of the sample-rate converter's definition, written from the definition:
the prototype g on the dense grid and the direct sum y[m] = sum_k x[k] g[m down - k up] -- no polyphase table, no kernel
code.  The upstream project has no resampler, so this IS the reference of the tests."""
from math import gcd

import numpy as np

RATE_OUT = 24000
RATES = (8000, 11025, 12000, 16000, 22050, 32000, 44100, 48000, 88200, 96000, 192000)
ZERO_CROSSINGS = 64
BETA = 10.06
MAX_UP, MAX_TAPS = 320, 1100


def plan(rate_in, rate_out=RATE_OUT):
    """(up, down, taps, half, n): n = floor(T fs) with T fs = 64 fs / (0.95 min(r, R)) taken in integers."""
    g = gcd(rate_in, rate_out)
    up, down = rate_out // g, rate_in // g
    fs = rate_in * up
    n = (20 * ZERO_CROSSINGS * fs) // (19 * min(rate_in, rate_out))
    half = -(-n // up)
    return up, down, 2 * half + 1, half, n


def bessel_i0(x):
    """sum_k ((x / 2)^k / k!)^2, all terms positive."""
    x = np.asarray(x, dtype=np.float64)
    q = 0.25 * x * x
    term = np.ones_like(x)
    total = np.ones_like(x)
    for k in range(1, 200):
        term = term * q / (k * k)
        total = total + term
    return total


def prototype(rate_in, rate_out=RATE_OUT):
    """g[i] for i = -n .. n (float64 [2 n + 1]) and n."""
    up, down, taps, half, n = plan(rate_in, rate_out)
    fs = rate_in * up
    low = min(rate_in, rate_out)
    fc = 0.95 * low / 2.0
    t_fs = ZERO_CROSSINGS * fs / (2.0 * fc)                     # T fs
    i = np.arange(-n, n + 1, dtype=np.float64)
    window = bessel_i0(BETA * np.sqrt(np.maximum(0.0, 1.0 - (i / t_fs) ** 2))) / bessel_i0(BETA)
    return up * (2.0 * fc / fs) * np.sinc(2.0 * fc * i / fs) * window, n


def table_from_prototype(rate_in, rate_out=RATE_OUT):
    """The polyphase storage table[p][t] = g[p + (t - half) up] (0 outside |i| <= n), float64 [up, taps]."""
    up, down, taps, half, n = plan(rate_in, rate_out)
    g, _ = prototype(rate_in, rate_out)
    idx = np.arange(up)[:, None] + (np.arange(taps)[None, :] - half) * up
    inside = np.abs(idx) <= n
    return np.where(inside, g[np.clip(idx + n, 0, 2 * n)], 0.0)


def output_length(length, rate_in, rate_out=RATE_OUT):
    up, down, _, _, _ = plan(rate_in, rate_out)
    return -(-int(length) * up // down)


def resample_at(x, rate_in, indices, rate_out=RATE_OUT, g_n=None, scale=1.0):
    """y[m] and b[m] = sum_k |x[k] g[m down - k up]| for the output indices ``indices`` of the signal(s) ``x`` [..., L]
    (any real dtype, multiplied by ``scale`` in float64 -- 1 / 32768 for int16 PCM; zero outside [0, L)).  Only the
    samples under the filter are touched, so a long input can be spot-checked.  Returns two float64 arrays
    [..., len(indices)]."""
    x = np.asarray(x)
    up, down, _, _, n = plan(rate_in, rate_out)
    g, n = g_n if g_n is not None else prototype(rate_in, rate_out)
    length = x.shape[-1]
    indices = np.asarray(indices, dtype=np.int64)
    y = np.zeros(x.shape[:-1] + (len(indices),))
    b = np.zeros_like(y)
    for at, m in enumerate(indices):
        centre = int(m) * down                                  # python integers: m down passes 2^31
        k_lo = max(0, -((n - centre) // up))                    # ceil((centre - n) / up)
        k_hi = min(length - 1, (centre + n) // up)
        if k_hi < k_lo:
            continue
        k = np.arange(k_lo, k_hi + 1, dtype=np.int64)
        coeff = g[centre - k * up + n]
        terms = (x[..., k_lo:k_hi + 1].astype(np.float64) * scale) * coeff
        y[..., at] = terms.sum(axis=-1)
        b[..., at] = np.abs(terms).sum(axis=-1)
    return y, b
