"""Plain numpy restatement of the per-channel energy normalisation: the definition evaluated
sequentially in float64 (``ref64``) and the two-launch scheme of include/seld_hip.h in float32 (``ref32``).  Nothing here
imports the package; the tests compare the device kernels and seld_native.pcen against it."""
import numpy as np

from standardise_ref import feature_like

CHUNK = 256          # SELD_PCEN_CHUNK_FRAMES
FRAME_RATE = 50.0    # feature frames per second (hop 480 at 24 kHz)

# (tau in seconds, alpha, delta, r, eps): the settings every comparison runs at
SETTINGS = ((0.4, 0.98, 2.0, 0.5, 1e-6), (0.4, 0.98, 2.0, 0.5, 1e-10), (0.06, 0.8, 10.0, 0.25, 1e-6), (2.0, 1.0, 2.0, 0.5, 1e-12))
# (N, T, C_log, C_total): one frame, one frame short of a chunk, exactly one chunk, one frame over, five chunks and a ragged
# sixth; a quarter, a half and one wavefront per frame row and two tiles
SHAPES = ((1, 1, 4, 4), (1, 255, 2, 3), (1, 256, 4, 7), (3, 257, 4, 7), (2, 1300, 8, 36))
# ref32's own error factor k against ref64 per setting, |y32 - y64| <= k (delta^r + |y64|), the largest over SHAPES with the
# inputs of ``inputs`` (tests/test_pcen_cpu.py::test_ref32_error_factors holds ref32 to them).  The device is allowed FOUR
# times its setting's value: its exp2 / log2 are 1-ulp instructions where numpy's are correctly rounded to within half
# an ulp or so, and a chunk carry may be folded in another, equally valid order.
REF32_K = (1.0e-6, 1.1e-6, 3.0e-7, 3.9e-6)      # measured 9.7e-7, 1.05e-6, 2.99e-7, 3.81e-6 (the last at T = 1300, tau = 2 s)
DEVICE_FACTOR = 4.0


def coefficient(tau):
    """s of a time constant tau in seconds at 50 frames per second, in float64: T_f = 50 tau,
    s = (sqrt(1 + 4 T_f^2) - 1) / (2 T_f^2)."""
    tf = FRAME_RATE * float(tau)
    return (np.sqrt(1.0 + 4.0 * tf * tf) - 1.0) / (2.0 * tf * tf)


def inputs(seed, N, T, C_log, C_total):
    """float32 [N, T, C_total, 64]: the first C_log channels like real log-mel (standardise_ref.feature_like: dB floored at
    -100 with runs of exact -100), the last of them raised by 60 dB so that loud and silent bands are both present; the other
    channels in [-1, 1]."""
    x = np.empty((N * T, C_total, 64), dtype=np.float32)
    x[:, :C_log] = feature_like(seed, N * T, 2 * C_log)[:, :C_log]
    x[:, C_log - 1] += np.float32(60.0)
    if C_total > C_log:
        rest = C_total - C_log
        x[:, C_log:] = feature_like(seed + 1, N * T, 2 * rest)[:, rest:]
    return x.reshape(N, T, C_total, 64)


def lattice_inputs(seed, N, T, C_log, C_total):
    """float32 [N, T, C_total, 64] whose log-mel channels lie on a 2^-10 dB lattice in [-70, +20): adding 20 dB is exact in
    float32 and neither version meets the -100 dB floor."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-1, 1, (N, T, C_total, 64)).astype(np.float32)
    steps = rng.integers(0, 90 * 1024, (N, T, C_log, 64))
    x[:, :, :C_log] = (steps.astype(np.float64) / 1024.0 - 70.0).astype(np.float32)
    return x


def ref64(x, c_log, s, alpha, delta, r, eps):
    """The definition, sequentially in float64: float64 [N, T, c_log, 64].  ``s`` as the device receives it (a float32 value)."""
    x = np.asarray(x)
    assert x.dtype == np.float32 and x.ndim == 4 and x.shape[3] == 64
    s = float(np.float32(s))
    alpha, delta, r, eps = (float(np.float32(v)) for v in (alpha, delta, r, eps))
    a = 1.0 - s
    e = np.exp2(x[:, :, :c_log].astype(np.float64) * (np.log2(10.0) / 10.0))
    y = np.empty_like(e)
    m = e[:, 0].copy()
    for t in range(x.shape[1]):
        m = a * m + s * e[:, t]
        y[:, t] = (e[:, t] * (eps + m) ** (-alpha) + delta) ** r - delta ** r
    return y


def _fma32(a, b, c):
    """fmaf of float32 operands: the product is exact in float64; the sum is rounded to float64 and then to float32 (a
    double rounding that differs from the fused one in about one case in 2^29)."""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(np.float32)


def ref32(x, c_log, s, alpha, delta, r, eps, chunk=CHUNK):
    """The two-launch scheme of include/seld_hip.h in float32: float32 [N, T, c_log, 64].  Every product, sum, exp2 and log2
    is rounded to float32 on its own, the smoother and the chunk carry are fused multiply-adds."""
    x = np.asarray(x)
    assert x.dtype == np.float32 and x.ndim == 4 and x.shape[3] == 64
    f = np.float32
    s, alpha, delta, r, eps = (f(v) for v in (s, alpha, delta, r, eps))
    a = f(f(1.0) - s)
    a_chunk = f(float(a) ** chunk)
    delta_r = f(float(delta) ** float(r))
    c = f(np.log2(10.0) / 10.0)
    T = x.shape[1]
    e = np.exp2(x[:, :, :c_log] * c)                          # float32 product, float32 exp2
    assert e.dtype == np.float32
    n_chunks = -(-T // chunk)
    # launch 1: the aggregate of every chunk that has a successor, from state 0
    agg = []
    for k in range(n_chunks - 1):
        m = np.zeros_like(e[:, 0])
        for t in range(k * chunk, (k + 1) * chunk):
            m = _fma32(a, m, s * e[:, t])
        agg.append(m)
    # launch 2: Horner over the earlier chunks from E[0], then the chunk's own frames
    y = np.empty_like(e)
    for k in range(n_chunks):
        m = e[:, 0].copy()
        for j in range(k):
            m = _fma32(a_chunk, m, agg[j])
        for t in range(k * chunk, min((k + 1) * chunk, T)):
            m = _fma32(a, m, s * e[:, t])
            gain = np.exp2(-alpha * np.log2(eps + m))
            y[:, t] = np.exp2(r * np.log2(e[:, t] * gain + delta)) - delta_r
    assert y.dtype == np.float32
    return y


def error_factor(y, y64, delta, r):
    """The smallest k with |y - y64| <= k (delta^r + |y64|) everywhere."""
    y64 = np.asarray(y64, dtype=np.float64)
    scale = float(np.float32(delta)) ** float(np.float32(r)) + np.abs(y64)
    return float((np.abs(np.asarray(y, dtype=np.float64) - y64) / scale).max())
