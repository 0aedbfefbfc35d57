"""Plain numpy restatement of the per-bin feature standardisation: the moments in exactly the
summation order include/seld_hip.h fixes, the finalisation, and the affine map in float32.  Nothing here imports the
package; the tests compare the device kernels and seld_standardise against it."""
import numpy as np

SLAB = 1024          # SELD_MOMENT_SLAB_FRAMES
FLAT_STD = 1e-6


def feature_like(seed, frames, channels):
    """Values like the real features: log-mel in dB floored at -100 with runs of exact -100, then channels in [-1, 1] with
    +0.0 and -0.0 mixed in."""
    rng = np.random.default_rng(seed)
    x = np.empty((frames, channels, 64), dtype=np.float32)
    mel = max(1, channels // 2)
    x[:, :mel] = np.maximum(rng.standard_normal((frames, mel, 64)) * 15 - 40, -100).astype(np.float32)
    for first in range(0, frames, 97):                       # a run of silence every 97 frames
        x[first:first + 13, :mel] = -100.0
    rest = rng.uniform(-1, 1, (frames, channels - mel, 64)).astype(np.float32)
    rest[rng.random(rest.shape) < 0.02] = 0.0
    rest[rng.random(rest.shape) < 0.02] = -0.0
    x[:, mel:] = rest
    return x


def moments(x, slab=SLAB):
    """x float32 [T, C, 64] -> float64 [2, C, 64] = (sum x, sum x * x): per slab of ``slab`` frames the row-wise fp64 sum in
    ascending frame order from 0.0, then the slab partials in ascending slab order from 0.0.  Every addition is one IEEE
    double addition; x * x of a widened float32 is exact in double."""
    x = np.asarray(x)
    assert x.dtype == np.float32 and x.ndim == 3
    total = np.zeros((2,) + x.shape[1:], dtype=np.float64)
    for first in range(0, x.shape[0], slab):
        acc = np.zeros_like(total)
        for t in range(first, min(first + slab, x.shape[0])):
            row = x[t].astype(np.float64)
            acc[0] += row
            acc[1] += row * row
        total += acc
    return total


def finalise(m, frames):
    """float64 moments -> (mean, std, scale32, shift32)."""
    m = np.asarray(m, dtype=np.float64)
    if not np.isfinite(m).all():
        raise ValueError("non-finite moments")
    mean = m[0] / frames
    var = np.maximum(m[1] / frames - mean * mean, 0.0)
    std = np.sqrt(var)
    flat = std < FLAT_STD
    safe = np.where(flat, 1.0, std)
    scale = np.where(flat, 1.0, 1.0 / safe).astype(np.float32)
    shift = np.where(flat, -mean, -mean / safe).astype(np.float32)
    return mean, std, scale, shift


def affine_exact_scale(v, scale, shift):
    """v * scale + shift in float32 for POWER-OF-TWO scales: the product is exact, so the sum's single rounding is the
    fused multiply-add's."""
    v, scale, shift = (np.asarray(a, dtype=np.float32) for a in (v, scale, shift))
    return (v * scale + shift).astype(np.float32)


def affine_f64(v, scale, shift):
    """The float64 evaluation x * s + b of float32 operands (the product exact, one double rounding in the sum)."""
    return np.asarray(v, dtype=np.float64) * np.asarray(scale, dtype=np.float64) + np.asarray(shift, dtype=np.float64)


def ulp32(reference):
    """The float32 unit in the last place at |reference| (float64 in), never below the smallest normal's."""
    mag = np.maximum(np.abs(np.asarray(reference, dtype=np.float64)), float(np.finfo(np.float32).tiny))
    _, exponent = np.frexp(mag)                          # mag = m * 2^exponent, m in [0.5, 1)
    return np.ldexp(1.0, exponent - 24)
