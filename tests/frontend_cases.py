"""Input families for the audio front end (csrc/logmel_core.h, logmel.hip, spatial.hip, nipd.hip): TEST INFRASTRUCTURE.

The front end packs two frames (t, t + 1 of one channel, t even) into one complex transform and runs four frames per
wavefront iteration; an all-zero frame's un-mixed spectrum is then the fp32 rounding residue of its partner unless the
kernel decides silence before the transform.  The families put digital silence next to LOUD frames in
every slot of that packing, on both load paths (reflecting edge iterations, interior iterations) and at both clip ends:

  loud_gap              one carrier in every channel (integer delays per channel), zero runs common to all channels
  loud_gap_one_channel  the same, the zero runs in some channels only (silent and sounding channels in one frame)
  full_scale_i16        int16 samples that reach -32768 and 32767, with a zero run
  scaled                a noise clip x and 2^-k x, k = 4, 10 (power-of-two scaling is exact in fp32)

Clips are short, L = 480 k + r: F = 1 + L // 480 runs over 2..9 (every F % 4, below and above one iteration; the interior
load path needs F >= 9) and 17, 18; r over 0, 1, 479.  Everything is deterministic.  tests/test_frontend_cases_cpu.py
asserts, in float64, that every family is what it claims to be.
"""
from dataclasses import dataclass
from functools import lru_cache

import numpy as np

HOP, N_FFT, SR = 480, 960, 24000
CARRIERS = ("tone_centre", "tone_between", "square", "clipped_noise")
DELAYS = (0, 1, 2, 3, -1, -2, 4, -3)             # samples, per channel (channel c = the carrier delayed by DELAYS[c])
DITHER_RMS = 0.003                               # noise floor under the tonal carriers: every bin of a sounding frame has power
PAD = 8                                          # carrier samples either side of the clip, for the delays

# (frames F, remainder r, all-zero frames): see the module docstring; frame t holds samples [480 (t - 1), 480 (t + 1)),
# reflected at the clip ends, so frame 0 is all-zero iff samples 0..480 are and frame 1 cannot be all-zero unless frame 0 is.
LAYOUTS = (
    (2, 479, (0,)),                              # first iteration = last: slot 0, the reflecting load path starts with zeros
    (3, 1, (2,)),                                # zero-padded clip end in slot 2, the partner lies past the end
    (4, 0, (3,)),                                # slot 3 of the only iteration
    (5, 479, (0, 4)),                            # one frame in the last, partial iteration
    (6, 1, (2, 5)),                              # slot 1 of the last, partial iteration (clip end), slot 2 of the first
    (7, 0, (3, 6)),
    (8, 479, (0, 4, 7)),
    (9, 0, (4, 7)),                              # F >= 9: iteration 1 (frames 4..7) takes the interior load path
    (9, 1, (5, 8)),
    (9, 479, (0, 6)),
    (17, 0, (7, 8, 12, 16)),                     # a zero run across the iteration boundary 7 | 8
    (18, 1, (0, 5, 8, 11, 14, 17)),              # either side of a boundary (11 | 12, 7 | 8), every slot, both clip ends
)


@dataclass(frozen=True)
class Case:
    family: str
    name: str
    pcm: np.ndarray                              # [C, L] float32, or int16 for full_scale_i16
    carrier: str
    delays: tuple = None                         # per channel, where a planted delay is the GCC-PHAT peak
    scale_log2: int = 0                          # 'scaled': this clip is 2^-scale_log2 times the family's base clip

    @property
    def frames(self):
        return 1 + self.pcm.shape[1] // HOP


def frame_sample_index(length):
    """[F, 960]: the sample that position n of frame t reads (center=True, reflect padding)."""
    padded = np.pad(np.arange(length), (N_FFT // 2, N_FFT // 2), mode="reflect")
    frames = 1 + length // HOP
    return padded[HOP * np.arange(frames)[:, None] + np.arange(N_FFT)[None, :]]


def dead_frames(pcm):
    """bool [C, F]: the frame's 960 padded samples are all zero."""
    idx = frame_sample_index(pcm.shape[1])
    return ~(np.asarray(pcm)[:, idx] != 0).any(axis=2)


def _zero(pcm, frames, channels=None):
    """Zero, in place, every sample that the given frames read (in the given channels, default all)."""
    idx = frame_sample_index(pcm.shape[1])
    for t in frames:
        cols = np.unique(idx[t])
        if channels is None:
            pcm[:, cols] = 0
        else:
            for c in channels:
                pcm[c, cols] = 0
    return pcm


def carrier(kind, length, seed):
    """float64 [length]: one of CARRIERS.  The tonal ones carry a noise floor of DITHER_RMS, so that no bin of a sounding
    frame is near the silence threshold (a pure tone at a bin centre has exact zeros everywhere else)."""
    rng = np.random.default_rng(seed)
    n = np.arange(length, dtype=np.float64)
    if kind == "tone_centre":                    # 1000 Hz = bin 40 exactly
        x = 0.9 * np.sin(2 * np.pi * 1000.0 * n / SR + 0.3)
    elif kind == "tone_between":                 # 1013 Hz = bin 40.52
        x = 0.9 * np.sin(2 * np.pi * 1013.0 * n / SR + 0.3)
    elif kind == "square":                       # +-0.9, period 24 samples
        x = np.where((n.astype(np.int64) % 24) < 12, 0.9, -0.9)
    elif kind == "clipped_noise":                # full scale: about a third of the samples clip
        return np.clip(rng.standard_normal(length), -1.0, 1.0 - 2.0 ** -15)
    else:
        raise ValueError(kind)
    return x + DITHER_RMS * rng.standard_normal(length)


def delayed(base, channels, length):
    """[C, length]: channel c = base delayed by DELAYS[c] samples (base has PAD extra samples either side)."""
    return np.stack([base[PAD - d:PAD - d + length] for d in DELAYS[:channels]])


@lru_cache(maxsize=None)
def loud_gap(channels, one_channel=False):
    """One Case per LAYOUTS row, the carriers in rotation.  ``one_channel``: the zero runs only in channels 1, 4, 7, ..."""
    cases = []
    for i, (frames, r, dead) in enumerate(LAYOUTS):
        length = HOP * (frames - 1) + r
        kind = CARRIERS[i % len(CARRIERS)]
        base = carrier(kind, length + 2 * PAD, 9000 + i)
        pcm = delayed(base, channels, length).astype(np.float32)
        gapped = [c for c in range(channels) if c % 3 == 1] if one_channel else None
        _zero(pcm, dead, gapped)
        family = "loud_gap_one_channel" if one_channel else "loud_gap"
        cases.append(Case(family, f"{family}-F{frames}-r{r}-{kind}-C{channels}", pcm, kind, DELAYS[:channels]))
    return tuple(cases)


def loud_gap_one_channel(channels):
    return loud_gap(channels, True)


@lru_cache(maxsize=None)
def full_scale_i16(channels):
    """int16 clips that reach both ends of the range: clipped noise (sigma 20000) and a -32768 / 32767 square wave of
    period 24 under a noise floor, each with zero runs (LAYOUTS rows of 9 and 18 frames)."""
    cases = []
    for i, (kind, row) in enumerate((("clipped_noise", 8), ("square", 11), ("clipped_noise", 4))):
        frames, r, dead = LAYOUTS[row]
        length = HOP * (frames - 1) + r
        rng = np.random.default_rng(9100 + i)
        n = np.arange(length + 2 * PAD)
        if kind == "square":
            base = np.where((n % 24) < 12, 32767.0, -32768.0) + 100.0 * rng.standard_normal(len(n))
        else:
            base = 20000.0 * rng.standard_normal(len(n))
        base = np.clip(np.rint(base), -32768, 32767)
        pcm = delayed(base, channels, length).astype(np.int16)
        _zero(pcm, dead)
        assert pcm.min() == -32768 and pcm.max() == 32767
        cases.append(Case("full_scale_i16", f"full_scale_i16-F{frames}-r{r}-{kind}-C{channels}", pcm, kind, DELAYS[:channels]))
    return tuple(cases)


SCALE_LOG2 = (0, 4, 10)


@lru_cache(maxsize=None)
def scaled(channels):
    """A noise clip (rms 0.4, independent channels but channel 1 = channel 0 delayed by 1) and its 2^-4 and 2^-10 copies,
    at 9 and at 6 frames.  A frame that the reflect padding makes symmetric about its centre -- frame 0 always, the last
    frame when r = 1 -- has a REAL spectrum, and a real Gaussian bin comes near zero a thousand times as often as a
    complex one: at 2^-10 such a frame cannot keep every bin 100 x above the silence threshold.  So samples 0..480 are
    zero (frame 0 is all-zero, in every copy) and r = 479."""
    cases = []
    for i, frames in enumerate((9, 6)):
        r = 479
        length = HOP * (frames - 1) + r
        rng = np.random.default_rng(9200 + i)
        # (the offset and the alternating term keep the two bins that are real in every frame, 0 and 480, away from zero)
        x = 0.4 * rng.standard_normal((channels, length + 1)) + 0.05 + 0.05 * (-1.0) ** np.arange(length + 1)
        x = np.clip(x, -1.0, 1.0 - 2.0 ** -15)
        x[1, 1:] = x[0, :-1]
        x = x[:, 1:].astype(np.float32)
        x[:, :HOP + 1] = 0.0
        for k in SCALE_LOG2:
            cases.append(Case("scaled", f"scaled-F{frames}-r{r}-k{k}-C{channels}", (x * np.float32(2.0 ** -k)).astype(np.float32),
                              "noise", None, k))
    return tuple(cases)


def as_float(case):
    """The clip as float32 in [-1, 1): int16 samples / 32768, as the kernels convert them."""
    if case.pcm.dtype == np.int16:
        return case.pcm.astype(np.float32) / np.float32(32768.0)
    return case.pcm
