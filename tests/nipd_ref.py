"""float64 numpy restatement of the mel-band NIPD feature (TEST INFRASTRUCTURE): the weight table,
NIPD from phasor words, NIPD from PCM through the oracle's STFT.  Nothing here calls the library's NIPD code.

  in range : k >= 1 and min_hz <= 25 k <= max_hz
  phi_m[k] = atan2(Im, Re) of conj(P_0[k]) P_m[k],  0 where either channel is silent
  nipd_m[j] = sum_k W[k][j] phi_m[k],  W[k][j] = fb[k][j] (-c / (2 pi f_k)) / sum_{k' in range} fb[k'][j]
"""
import ctypes
from pathlib import Path

import numpy as np

from oracle import features as ofeat

N_BINS, N_MELS, MAX_TAPS, BIN_HZ = 481, 64, 48, 25.0
SILENCE_POWER = ofeat.GCC_SILENCE_POWER              # the phasor pass stores 0 for |X|^2 at or below this
LIB = Path(__file__).resolve().parent.parent / "sound-event-localization-detection_amd" / "libseld_hip.so"


def library_filterbank() -> np.ndarray:
    """The library's fp32 HTK filterbank [481, 64] (seld_default_tables, a host function): a constant of the method."""
    fb = np.zeros((N_BINS, N_MELS), dtype=np.float32)
    lib = ctypes.CDLL(str(LIB))
    lib.seld_default_tables.argtypes = [ctypes.c_void_p] * 5
    assert lib.seld_default_tables(None, fb.ctypes.data, None, None, None) == 0
    return fb


def in_range(min_hz: float, max_hz: float) -> np.ndarray:
    f = BIN_HZ * np.arange(N_BINS)
    return (np.arange(N_BINS) >= 1) & (f >= min_hz) & (f <= max_hz)


def dense_weights(fb: np.ndarray, min_hz: float, max_hz: float, speed: float) -> np.ndarray:
    """W [481, 64] in float64, the band sums taken in ascending k."""
    fb = np.asarray(fb, dtype=np.float64)
    ok = in_range(min_hz, max_hz)
    w = np.zeros((N_BINS, N_MELS))
    for j in range(N_MELS):
        den = 0.0
        for k in range(N_BINS):
            if ok[k]:
                den += fb[k, j]
        if den == 0.0:
            continue
        for k in range(1, N_BINS):
            if ok[k]:
                w[k, j] = fb[k, j] * (-speed / (2.0 * np.pi * BIN_HZ * k)) / den
    return w


def sparse_table(fb: np.ndarray, min_hz: float, max_hz: float, speed: float):
    """(first_bin int [64], taps int [64], w float64 [64, 48]) of the dense weights: a band's non-zero weights are
    contiguous; an empty band has first_bin = taps = 0."""
    dense = dense_weights(fb, min_hz, max_hz, speed)
    first, taps, w = np.zeros(N_MELS, dtype=np.int64), np.zeros(N_MELS, dtype=np.int64), np.zeros((N_MELS, MAX_TAPS))
    for j in range(N_MELS):
        ks = np.nonzero(dense[:, j])[0]
        if len(ks) == 0:
            continue
        assert len(ks) == ks[-1] - ks[0] + 1 <= MAX_TAPS
        first[j], taps[j] = ks[0], len(ks)
        w[j, :len(ks)] = dense[ks, j]
    return first, taps, w


def words_to_int(words: np.ndarray):
    """Phasor words (re | im << 16, two signed 16-bit numbers) -> (re, im) as int64."""
    u = np.asarray(words).astype(np.int64) & 0xFFFFFFFF
    re, im = u & 0xFFFF, u >> 16
    return np.where(re >= 32768, re - 65536, re), np.where(im >= 32768, im - 65536, im)


def nipd_from_words(words: np.ndarray, weights: np.ndarray) -> np.ndarray:
    """words [C, F, >= 481] -> nipd [C - 1, F, 64] in float64 with the dense weights [481, 64]."""
    re, im = words_to_int(np.asarray(words)[..., :N_BINS])
    silent = (re == 0) & (im == 0)
    out = []
    for m in range(1, re.shape[0]):
        pr = re[0] * re[m] + im[0] * im[m]
        pi = re[0] * im[m] - im[0] * re[m]
        phi = np.arctan2(pi.astype(np.float64), pr.astype(np.float64))
        phi[silent[0] | silent[m]] = 0.0
        out.append(phi @ weights)
    return np.stack(out)


def pcm_phase(pcm: np.ndarray, q15: bool = False):
    """[C, L] -> phi [C - 1, F, 481] from the float64 STFT; ``q15``: through the rounding of the phasor words (each unit
    phasor's components scaled by 32767 and rounded to nearest)."""
    spec = np.swapaxes(ofeat.stft_f64(np.asarray(pcm, dtype=np.float64)), -1, -2)        # [C, F, 481]
    power = spec.real ** 2 + spec.imag ** 2
    silent = power <= SILENCE_POWER
    if q15:
        unit = spec / np.sqrt(np.where(silent, 1.0, power))
        re, im = np.rint(unit.real * 32767.0), np.rint(unit.imag * 32767.0)
        re[silent] = im[silent] = 0.0
        spec = re + 1j * im
    out = []
    for m in range(1, spec.shape[0]):
        r = np.conj(spec[0]) * spec[m]
        phi = np.arctan2(r.imag, r.real)
        phi[silent[0] | silent[m]] = 0.0
        out.append(phi)
    return np.stack(out)


def nipd_from_pcm(pcm: np.ndarray, weights: np.ndarray, q15: bool = False) -> np.ndarray:
    """[C, L] -> nipd [C - 1, F, 64] in float64."""
    return pcm_phase(pcm, q15) @ weights


DELAYS = (0, 1, 2, 3, 4, 5, -1, -2)                  # samples, per channel; channel 0 is the reference


def delayed_noise(length: int = 9600, seed: int = 77) -> np.ndarray:
    """[8, length] float32: one noise sequence cut at the integer delays DELAYS (channel c = the sequence delayed by
    DELAYS[c] samples)."""
    pad = 8
    base = ofeat.synth_pcm(seed, 1, length + 2 * pad, "noise")[0].numpy()
    return np.stack([base[pad - d:pad - d + length] for d in DELAYS]).astype(np.float32)
