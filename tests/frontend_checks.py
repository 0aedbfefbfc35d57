"""Assertions on the front end's outputs for the families of tests/frontend_cases.py, shared by the CPU tests (which feed
them the lane emulator's words and spectra) and the GPU tests (tests/test_frontend_edges_gpu.py).  References: oracle/
features.py and tests/nipd_ref.py in float64, computed once per case and never changed.

What a frame is held to:

  all-zero frame (its 960 padded samples are zero in the channels involved)
      EXACT: spectrum 0 + 0j, phasor word 0, log-mel -100.0, intensity 0.0, NIPD 0.0; GCC-PHAT the unit pulse at lag 0
      to PULSE_TOL = 2e-5 (the bar tests/test_spatial_gpu.py holds the exact route to: the fp16 table's rounding).
  every other frame
      the stated bar of the feature (BAR below), or -- where the fp32 STFT itself cannot do better -- 4 x the error of
      the fp32 peer: the same feature computed with the oracle's formulas in float64 from torch.stft's fp32 spectrum of
      the same input (the rule and the factor of tests/test_logmel_gpu.py test_tones_and_silence_against_float64).  In a
      frame that one tone dominates most bins lie far under the peak, and there any two fp32 transforms disagree in phase.
      The Q15 phasor words add a rounding of 1 / (2 * 32767) per component that the peer does not have; its worst case is
      bounded here, per feature, and added to the peer term -- never to the bar:
          tolerance = max(BAR, 4 * peer_error + q15_bound)

No measured constant enters a bound.
"""
from functools import lru_cache

import numpy as np
import torch

import frontend_cases as fc
import nipd_ref
from oracle import features as ofeat

BAR = {"gcc": 1e-4, "nipd": 1e-4, "iv": 1e-4}        # tests/test_spatial_gpu.py, tests/test_nipd_gpu.py (end to end)
PULSE_TOL = 2e-5
STFT_REL = 2e-6                                      # tests/test_spatial_gpu.py test_stft_matches_torch_stft, per frame here
PEER_FACTOR = 4.0
SENTINEL = -12345.0
SPEED, NIPD_LO, NIPD_HI = 343.0, 50.0, 2000.0

# One Q15 component is off by at most half a step, the phasor by sqrt(2) times that, its angle by asin of it; the
# product of two words by twice that.
Q15_ANGLE = 2.0 * np.arcsin(np.sqrt(2.0) * 0.5 / 32767.0)
# GCC-PHAT: cc[lag] = (1 / 960) sum over 960 bins (2 / 960 over the 481 of the half spectrum) of a unit factor whose
# angle is off by at most Q15_ANGLE: |exp(i a) - exp(i b)| <= |a - b|.
GCC_Q15_BOUND = 2.0 / 960.0 * 481.0 * Q15_ANGLE


def nipd_weights():
    return nipd_ref.dense_weights(nipd_ref.library_filterbank(), NIPD_LO, NIPD_HI, SPEED)


def nipd_q15_bound(weights):
    """Each bin's phase is off by at most Q15_ANGLE: the band's value by that times the band's sum of |weights|."""
    return float(Q15_ANGLE * np.abs(weights).sum(axis=0).max())


def pairs(channels):
    return [(m, n) for m in range(channels) for n in range(m + 1, channels)]


# ---------------------------------------------------------------------------------------------------- the formulas

def gcc_from_spec(spec):
    """oracle.features.gcc_phat_f64's formula on a given spectrum [C, 481, F] -> [pairs, 64, F]."""
    spec = np.asarray(spec, dtype=np.complex128)
    power = spec.real ** 2 + spec.imag ** 2
    out = []
    for m, n in pairs(spec.shape[0]):
        phase = np.exp(1j * np.angle(np.conj(spec[m]) * spec[n]))
        phase[(power[m] <= ofeat.GCC_SILENCE_POWER) | (power[n] <= ofeat.GCC_SILENCE_POWER)] = 1.0
        cc = np.fft.irfft(phase, n=ofeat.N_FFT, axis=0)
        out.append(np.concatenate((cc[-32:], cc[:32]), axis=0))
    return np.stack(out)


def iv_from_spec(spec, eps=1e-8):
    """oracle.features.foa_intensity_f64's formula on a given spectrum [4, 481, F] -> [3, 64, F]."""
    spec = np.asarray(spec, dtype=np.complex128)
    w, xyz = spec[0], spec[1:]
    energy = eps + np.abs(w) ** 2 + (np.abs(xyz) ** 2).sum(0) / 3.0
    fb = ofeat.mel_filterbank_htk().numpy().astype(np.float64)
    return np.einsum("cft,fm->cmt", np.real(np.conj(w)[None] * xyz) / energy[None], fb)


def nipd_from_spec(spec, weights):
    """tests/nipd_ref.py pcm_phase's formula on a given spectrum [C, 481, F] -> [C - 1, F, 64]."""
    spec = np.swapaxes(np.asarray(spec, dtype=np.complex128), -1, -2)              # [C, F, 481]
    silent = spec.real ** 2 + spec.imag ** 2 <= nipd_ref.SILENCE_POWER
    out = []
    for m in range(1, spec.shape[0]):
        r = np.conj(spec[0]) * spec[m]
        phi = np.arctan2(r.imag, r.real)
        phi[silent[0] | silent[m]] = 0.0
        out.append(phi @ weights)
    return np.stack(out)


def words_to_spec(words):
    """Phasor words [C, F, >= 481] -> unit (or zero) complex spectrum [C, 481, F]."""
    re, im = nipd_ref.words_to_int(np.asarray(words)[..., :481])
    return np.swapaxes((re + 1j * im) / 32767.0, -1, -2)


# ---------------------------------------------------------------------------------------------------- references

class Reference:
    """Everything float64 says about one case, and what the fp32 peer says: computed once."""

    def __init__(self, case):
        self.case = case
        self.x = fc.as_float(case)                                                 # float32 [C, L]
        x64 = self.x.astype(np.float64)
        self.dead = fc.dead_frames(case.pcm)                                       # [C, F]
        self.spec = ofeat.stft_f64(x64)                                            # [C, 481, F]
        self.spec[:, :, :][np.broadcast_to(self.dead[:, None, :], self.spec.shape)] = 0.0     # (it is: -0.0 and 0j apart)
        self.peer_spec = ofeat.stft_torch(torch.from_numpy(self.x)).numpy().astype(np.complex128)
        self.logmel32 = ofeat.logmel_torch(torch.from_numpy(self.x)).numpy()       # [C, 64, F]: the CPU path, the log-mel bar's reference
        self.channels, self.frames = self.dead.shape

    @property
    def all_dead(self):
        """Frames that are all-zero in every channel."""
        return self.dead.all(axis=0)

    @lru_cache(maxsize=None)
    def gcc(self):
        return gcc_from_spec(self.spec), gcc_from_spec(self.peer_spec)

    @lru_cache(maxsize=None)
    def iv(self):
        return iv_from_spec(self.spec[:4]), iv_from_spec(self.peer_spec[:4])

    @lru_cache(maxsize=None)
    def nipd(self):
        w = nipd_weights()
        return nipd_from_spec(self.spec, w), nipd_from_spec(self.peer_spec, w)


@lru_cache(maxsize=None)
def reference(case_name, family, channels):
    for case in family(channels):
        if case.name == case_name:
            return Reference(case)
    raise KeyError(case_name)


def ref_of(case, family):
    return reference(case.name, family, case.pcm.shape[0])


def _tolerance(kind, ref, peer, select, q15_bound):
    peer_err = float(np.abs(peer - ref)[select].max()) if select.any() else 0.0
    return max(BAR[kind], PEER_FACTOR * peer_err + q15_bound), peer_err


# ---------------------------------------------------------------------------------------------------- the checks
# Every check returns the figures it measured (for the tests to print) after asserting.

def check_stft(r, got):
    """got: complex [C, F, 481].  All-zero frames exactly 0 + 0j; every other frame within STFT_REL of float64, relative
    to ITS OWN largest bin (a loud neighbour must not hide a quiet frame's error)."""
    got = np.asarray(got)
    assert got.shape == (r.channels, r.frames, 481)
    assert np.isfinite(got.view(np.float32)).all()
    ref = np.swapaxes(r.spec, -1, -2)
    assert not got[r.dead].real.any() and not got[r.dead].imag.any(), "an all-zero frame's spectrum is not exactly 0"
    live = ~r.dead
    scale = np.abs(ref).max(axis=2)                                                # [C, F]
    err = np.abs(got - ref).max(axis=2)
    worst = float((err[live] / scale[live]).max())
    assert worst <= STFT_REL, f"{r.case.name}: worst per-frame |X - X64| / max|X64| = {worst:.3e}"
    return {"stft_rel": worst}


def check_logmel(r, got):
    """got: [C, 64, F] dB.  All-zero frames exactly -100.0; the others to the log-mel bar (tests/logmel_checks.py)."""
    from logmel_checks import assert_logmel_close
    got = np.asarray(got)
    assert got.shape == (r.channels, 64, r.frames)
    dead = np.broadcast_to(r.dead[:, None, :], got.shape)
    assert (got[dead] == -100.0).all(), f"{r.case.name}: an all-zero frame is not exactly -100 dB"
    assert (r.logmel32[dead] == -100.0).all()
    worst, _ = assert_logmel_close(got, r.logmel32)
    return {"logmel_db": worst}


def check_gcc(r, got, q15):
    """got: [pairs, 64, F].  Frames that are all-zero in every channel: the unit pulse to PULSE_TOL.  Frames with a silent
    channel among sounding ones: the bar.  Fully sounding frames: max(bar, 4 x peer + Q15 bound).  The planted delay is
    the peak of every pair in every frame whose neighbours (t - 1 .. t + 1) are sounding too, first and last frame apart."""
    got = np.asarray(got, dtype=np.float64)
    ref, peer = r.gcc()
    assert got.shape == ref.shape and np.isfinite(got).all()
    out = {}
    pulse = np.zeros(64)
    pulse[32] = 1.0
    if r.all_dead.any():
        out["pulse"] = float(np.abs(got[:, :, r.all_dead] - pulse[None, :, None]).max())
        assert out["pulse"] <= PULSE_TOL, f"{r.case.name}: all-zero frames are {out['pulse']:.3e} from the unit pulse"
    some = r.dead.any(axis=0) & ~r.all_dead
    if some.any():
        out["mixed"] = float(np.abs(got - ref)[:, :, some].max())
        assert out["mixed"] <= BAR["gcc"], f"{r.case.name}: frames with a silent channel: {out['mixed']:.3e}"
        for p, (m, n) in enumerate(pairs(r.channels)):                             # pairs with the silent channel: the pulse
            t = r.dead[m] | r.dead[n]
            if t.any():
                assert np.abs(got[p][:, t] - pulse[:, None]).max() <= PULSE_TOL, (r.case.name, m, n)
    sounding = ~r.dead.any(axis=0)
    select = np.broadcast_to(sounding[None, None, :], ref.shape)
    tol, peer_err = _tolerance("gcc", ref, peer, select, GCC_Q15_BOUND if q15 else 0.0)
    out["sounding"] = float(np.abs(got - ref)[select].max())
    out["peer"], out["tol"] = peer_err, tol
    assert out["sounding"] <= tol, f"{r.case.name}: {out['sounding']:.3e} > {tol:.3e} (fp32 peer {peer_err:.3e})"
    if r.case.delays is not None:
        for t in range(1, r.frames - 1):
            if sounding[t - 1:t + 2].all():
                for p, (m, n) in enumerate(pairs(r.channels)):
                    want = 32 + r.case.delays[n] - r.case.delays[m]
                    assert got[p, :, t].argmax() == want, (r.case.name, t, (m, n), int(got[p, :, t].argmax()), want)
    return out


def check_iv(r, got):
    """got: [3, 64, F].  Frames that are all-zero in every channel: exactly 0.  The others: max(bar, 4 x peer)."""
    got = np.asarray(got, dtype=np.float64)
    ref, peer = r.iv()
    assert got.shape == ref.shape and np.isfinite(got).all()
    assert not got[:, :, r.all_dead].any(), f"{r.case.name}: an all-zero frame's intensity is not exactly 0"
    select = np.broadcast_to(~r.all_dead[None, None, :], ref.shape)
    tol, peer_err = _tolerance("iv", ref, peer, select, 0.0)
    worst = float(np.abs(got - ref)[select].max())
    assert worst <= tol, f"{r.case.name}: {worst:.3e} > {tol:.3e} (fp32 peer {peer_err:.3e})"
    return {"iv": worst, "peer": peer_err, "tol": tol}


def check_nipd(r, got):
    """got: [C - 1, F, 64].  A frame in which channel 0 or channel m is all-zero: nipd_m exactly 0.  The other INNER frames:
    max(bar, 4 x peer + Q15 bound).  The first frame (always) and the last (when L % 480 is 1) are symmetric about their
    centre under reflect padding: their spectra are real, every phase difference is 0 or +-pi, and which of +pi / -pi it is
    hangs on the sign of a rounding error -- the bar of tests/test_nipd_gpu.py is stated on the inner frames for that
    reason, and so is this one."""
    got = np.asarray(got, dtype=np.float64)
    ref, peer = r.nipd()
    assert got.shape == ref.shape and np.isfinite(got).all()
    zero = r.dead[0][None, :] | r.dead[1:]                                         # [C - 1, F]
    assert not got[zero].any(), f"{r.case.name}: NIPD of an all-zero frame is not exactly 0"
    assert not ref[zero].any()
    inner = np.zeros(r.frames, dtype=bool)
    inner[1:-1] = True                                                             # (as tests/test_nipd_gpu.py: see the docstring)
    select = np.broadcast_to((~zero & inner[None, :])[:, :, None], ref.shape)
    tol, peer_err = _tolerance("nipd", ref, peer, select, nipd_q15_bound(nipd_weights()))
    worst = float(np.abs(got - ref)[select].max()) if select.any() else 0.0
    assert worst <= tol, f"{r.case.name}: {worst:.3e} m > {tol:.3e} m (fp32 peer {peer_err:.3e} m)"
    return {"nipd": worst, "peer": peer_err, "tol": tol}


def check_words_dead(r, words):
    """words: int [C, F, pitch].  All-zero frames: word 0 in every bin; bins 481.. of every row untouched (-1)."""
    words = np.asarray(words)
    assert not words[r.dead][:, :481].any(), f"{r.case.name}: an all-zero frame has non-zero phasor words"
    assert (words[..., 481:] == -1).all()
    assert words[~r.dead][:, :481].any(axis=1).all()
