"""Seeded inputs and the recorded-result keys shared by tools/record_frontend_parent_golden.py and
tests/test_frontend_parent_bits_gpu.py (no test in here).

Clip lengths, the smallest that reach every path of csrc/logmel.hip:
  6277   14 frames, 4 iterations per row: 1-2 interior, 0 an edge, 3 an edge with two of its four frames (F % 4 == 2)
  2000   5 frames, no interior iteration: the stand-alone logmel_edge_kernel launch
  481    the minimum, one iteration
Every family runs at both PCM types.  Channel C - 1 of clip 0 is all zero, and channel 1 of clip 1 has two zero blocks,
samples [0, 960) -- frames 0 and 1, the packed pair of an edge iteration -- and [1440, 2880) -- frames 4 and 5, the
packed pair of an interior one -- so that the any_dead branches of every kernel run."""
import hashlib

import numpy as np
import torch

LENGTHS = (6277, 2000, 481)
DTYPES = (torch.float32, torch.int16)
SEED = 29
HASH_ABOVE = 64 * 1024          # bytes: larger results are recorded as shape, dtype and SHA-256
ZERO_BLOCKS = ((0, 960), (1440, 2880))
FILL = -7.0                     # what a strided placement must leave around the channels it writes
SAME_LOGMEL = ("logmel_gcc_c3", "logmel_nipd_c3")       # their channels 0..2 are those of "phasors_logmel", bit for bit


def pcm(n, c, length, dtype):
    """[n, c, length] host PCM, float32 in [-1, 1) or the int16 rounding of it, with the zero channel and zero blocks."""
    g = torch.Generator().manual_seed(SEED + 1000 * c + length)
    x = torch.rand(n, c, length, generator=g) * 1.6 - 0.8
    x[0, c - 1] = 0.0
    for lo, hi in ZERO_BLOCKS:
        if n > 1 and hi <= length:
            x[1, 1, lo:hi] = 0.0
    return x if dtype == torch.float32 else torch.round(x * 32767.0).to(torch.int16)


def _suffix(dtype):
    return "f32" if dtype == torch.float32 else "i16"


def run(nat, device, length, dtype):
    """Every front-end family on the seeded clips of ``length`` samples: a dict name -> device tensor (float32 or int32)."""
    lib, p, sfx = nat.load_library(), nat._p, _suffix(dtype)
    frames, pitch = nat.num_frames(length), int(nat.load_library().seld_phasor_pitch())
    out = {}
    x3 = pcm(2, 3, length, dtype).to(device)
    nat.ensure_init(device)
    stream = nat._stream_ptr(device)
    # the log-mel kernels: 12 interior iterations at 6277 samples, split over two wavefronts, C = 3
    out["logmel_cft"] = nat.logmel(x3, "cft")
    out["logmel_tcf"] = nat.logmel(x3, "tcf")
    wide = torch.full((2, frames, 5, 64), FILL, device=device)           # channels 1..3 of a wider time-major tensor
    s_n, s_t, s_c, s_m = wide.stride()
    nat.check(getattr(lib, f"seld_logmel_{sfx}_strided")(p(x3), 2, 3, length, p(wide[:, :, 1:]), s_n, s_c, s_m, s_t, stream))
    out["logmel_strided"] = wide
    mel = torch.empty(2, frames, 3, 64, device=device)
    s_n, s_t, s_c, s_m = mel.stride()
    words = torch.zeros(2, 3, frames, pitch, dtype=torch.int32, device=device)     # (words 481..487 of a row are never written)
    nat.check(getattr(lib, f"seld_logmel_phasors_{sfx}")(p(x3), 2, 3, length, p(mel), s_n, s_c, s_m, s_t, p(words), stream))
    out["phasors_logmel"], out["phasors_words"] = mel, words
    # the spectrum export and the STFT, C = 2
    x2 = pcm(2, 2, length, dtype).to(device)
    mel = torch.empty(2, frames, 2, 64, device=device)
    s_n, s_t, s_c, s_m = mel.stride()
    spec = torch.empty(2, 2, frames, 481, 2, device=device)
    nat.check(getattr(lib, f"seld_logmel_spectrum_{sfx}")(p(x2), 2, 2, length, p(mel), s_n, s_c, s_m, s_t, p(spec), stream))
    out["spectrum_logmel"], out["spectrum_spec"] = mel, spec
    out["stft"] = torch.view_as_real(nat.stft(x2))
    # the fused FOA pass and the default microphone-array features
    out["logmel_iv"] = nat.spatial_features(pcm(2, 4, length, dtype).to(device), "logmel_iv")
    out["logmel_gcc_c3"] = nat.spatial_features(x3, "logmel_gcc")
    out["logmel_gcc_c7"] = nat.spatial_features(pcm(2, 7, length, dtype).to(device), "logmel_gcc")    # 21 pairs: two tiles
    out["logmel_nipd_c3"] = nat.spatial_features(x3, "logmel_nipd")
    torch.cuda.synchronize(device)
    return out


def key(length, dtype, name):
    return f"L{length}_{_suffix(dtype)}_{name}"


def bits(x):
    """The bit patterns of a float32 / int32 device tensor as a uint32 numpy array."""
    return x.contiguous().view(torch.int32).cpu().numpy().view(np.uint32)


def record(name, x):
    """What the fixture keeps of a result: its bit patterns, or above HASH_ABOVE bytes the words [shape..., dtype (0 float32,
    1 int32), SHA-256 of the bytes as 8 words].  Of the SAME_LOGMEL results it keeps the spatial channels only: their
    log-mel channels come from the same call on the same clips as "phasors_logmel", which the test compares them with."""
    b = bits(x[:, :, 3:] if name in SAME_LOGMEL else x)
    if b.nbytes <= HASH_ABOVE:
        return b
    digest = np.frombuffer(hashlib.sha256(b.tobytes()).digest(), dtype=np.uint32)
    return np.concatenate([np.asarray(b.shape + (int(x.dtype == torch.int32),), dtype=np.uint32), digest])
