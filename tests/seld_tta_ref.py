"""Float64 CPU restatement of test-time augmentation in the SELD decode and the inputs its tests
share -- TEST infrastructure only; the product (seld_eval.py, csrc/seld_tta.hip) never imports it."""
from functools import lru_cache

import numpy as np

import seld_eval_ref as ref

SEG = np.array([[0, 57], [57, 46]])        # 3 windows, 22 meta-frames: partial meta-frames (2 and 1 frames), one that
TOTAL = 103                                # straddles a window start (frames 97..101), a segment boundary in a window
THRESHOLD = 0.5
# (dtype, seed, patterns) of the planted cases; every list holds a pattern with an odd quarter turn and no mirror
# (2, 3, 6, 7): lists of involutions only cannot tell cell_dest from cell_source
CASES = {"bf16-all": ("bf16", 2235, tuple(range(16))),
         "fp32-three": ("fp32", 2234, (2, 6, 11)),
         "fp32-one": ("fp32", 2236, (3,))}


def _bf16_round(x):
    """float32 -> the nearest bfloat16 values, as float32."""
    import torch
    return torch.from_numpy(x).to(torch.bfloat16).float().numpy()


def planted_tta(seed, patterns, bf16):
    """float32 [P, W, 250, 648, 14]: stack n is the planted logits of the plain decode test as the model would give them
    for the sound field transformed by pattern p_n (an event of cell x shows at cell_dest(p_n)[x]) plus the stack's own
    N(0, 0.5); rounded to bfloat16 values when ``bf16``."""
    import seld_augment
    base = ref.planted_logits(SEG, seed)
    out = np.empty((len(patterns),) + base.shape, dtype=np.float32)
    for n, p in enumerate(patterns):
        noise = np.random.default_rng([seed, p]).normal(0.0, 0.5, base.shape).astype(np.float32)
        out[n] = base[:, :, seld_augment.cell_source(p), :] + noise
    return _bf16_round(out) if bf16 else out


def decode_probs_tta(x, patterns):
    """P_q [Q, 648, 13] in float64: the mean over the stacks of the plain restatement of each un-permuted stack."""
    import seld_augment
    acc = 0.0
    for n, p in enumerate(patterns):
        acc = acc + ref.decode_probs(x[n][:, :, seld_augment.cell_dest(p), :], SEG, TOTAL)
    return acc / len(patterns)


@lru_cache(maxsize=None)
def case(name):
    """(dtype name, patterns, logits float32 [P, 3, 250, 648, 14], float64 P_q [22, 648, 13]) of a planted case, computed
    once per process and shared; do not write to the arrays."""
    dtype, seed, patterns = CASES[name]
    x = planted_tta(seed, patterns, dtype == "bf16")
    want = decode_probs_tta(x, patterns)
    want.setflags(write=False)
    return dtype, patterns, x, want


def rows_for_clip(rng, n_frames):
    """Synthetic CSV rows: 0-3 events per meta-frame at distinct cells, same-class sources >= 2 cells apart (azimuth
    wraps), integer DOAs inside their cell, no duplicates; plus rows with 5 m >= n that the evaluation must drop."""
    n_meta = (n_frames + 4) // 5
    rows = []
    for m in range(n_meta):
        placed = []
        for src in range(int(rng.integers(0, 4))):
            for _ in range(100):
                c, i, j = int(rng.integers(0, 13)), int(rng.integers(0, 18)), int(rng.integers(0, 36))
                ok = True
                for c2, i2, j2 in placed:
                    dj = min(abs(j - j2), 36 - abs(j - j2))
                    if (i, j) == (i2, j2) or (c == c2 and max(abs(i - i2), dj) < 2):
                        ok = False
                if ok:
                    placed.append((c, i, j))
                    rows.append([m, c, src, -180 + 10 * j + int(rng.integers(0, 10)), -90 + 10 * i + int(rng.integers(0, 10))])
                    break
    for extra in range(3):
        rows.append([n_meta + 2 * extra, int(rng.integers(0, 13)), 0, 0, 0])
    return np.array(rows, dtype=np.int64).reshape(-1, 5)


def two_clip_dataset(gpu_device, seed):
    """Two noise clips (7 s and 4 s, odd lengths) with synthetic rows: (dataset, rows, frame counts)."""
    import dataset
    from oracle import features as ofeat
    lengths = (24000 * 7 + 1234, 24000 * 4 + 517)
    clips = [ofeat.synth_pcm(i + seed, 4, n, "noise") for i, n in enumerate(lengths)]
    rng = np.random.default_rng(seed)
    frames = [min(1 + n // 480, dataset.label_frame_count(n / 24000)) for n in lengths]
    rows = [rows_for_clip(rng, f) for f in frames]
    ds = dataset.SELDDataset.from_pcm(clips, rows, device=gpu_device, use_gaussian_augmentation=False)
    return ds, rows, frames
