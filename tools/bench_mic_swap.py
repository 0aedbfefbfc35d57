#!/usr/bin/env python
"""Cost of the channel swap of microphone-array features in the device window gather (csrc/micswap.hip; DESIGN.md section
25), on the GPU.

  python tools/bench_mic_swap.py                 one JSON document (also --out FILE, e.g. profiles/mic_swap.json)

At the training shape (B = 32 windows of 250 frames) and the two 'logmel_gcc' widths -- 10 channels (the tetrahedron) and 36
(the cube, 8 microphones) -- the array gather (gather_mic_kernel) against the augmenting gather (gather_augment_kernel with an
identity channel table: what an array got before its geometry was known) on the same buffers, starts and parameter rows,
alternating in one process, measured as tools/bench_augment.py measures: a timed sample is a burst of launches captured as
one HIP graph and replayed between two device events, every launch of a burst with its own random starts and rows, on a
timeline larger than the Infinity Cache.  Cases: identity patterns (the cost of the kernel form itself) and the drawn
case (AUGMENT_SPATIAL over the array's symmetries, two time and two frequency masks), where about half the GCC-PHAT
channels of a moved window are reversed.  Both kernels read and write every byte once: 2 units per window.
"""
import argparse
import json
import statistics
import sys
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
for p in (str(ROOT), str(ROOT / "sound-event-localization-detection_amd"), str(ROOT / "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

from bench_augment import Burst  # noqa: E402  (the captured burst of launches, shared with the augmentation's bench)

B, WINDOW = 32, 250
HBM_PEAK = 8.0e12
CASES = ("identity", "drawn")
DRAWN = dict(AUGMENT_SPATIAL=True, AUGMENT_TIME_MASKS=2, AUGMENT_TIME_MASK_MAX=40, AUGMENT_FREQ_MASKS=2, AUGMENT_FREQ_MASK_MAX=12)


def arrays():
    import seld_augment
    cube = [(x, y, z) for x in (-0.05, 0.05) for y in (-0.05, 0.05) for z in (-0.05, 0.05)]
    return {10: seld_augment.mic_positions("tetra_starss"), 36: seld_augment.mic_positions(cube)}


def bench_kernels(dev, channels, positions, frames, bursts, burst_len):
    import seld_augment
    import seld_native as nat
    rng = np.random.default_rng(channels)
    mics = len(positions)
    perm = seld_augment.mic_permutations(positions)
    identity = np.tile(np.arange(channels, dtype=np.uint8), (16, 1))
    spec_tm = torch.randn(frames, channels, 64, device=dev)
    out = torch.empty(B, WINDOW, channels, 64, device=dev)
    unit = out.numel() * 4
    result = {"channels": channels, "microphones": mics, "valid_patterns": list(seld_augment.mic_valid_patterns(positions)),
              "timeline_frames": frames, "bytes_per_unit": unit, "bursts": bursts, "launches_per_burst": burst_len, "cases": {}}
    for case in CASES:
        launches, moved = [], []
        for _ in range(burst_len):
            rows = seld_augment.identity_rows(B)
            if case == "drawn":
                cfg = SimpleNamespace(MIC_POSITIONS=positions, **DRAWN)
                rows = seld_augment.draw(int(rng.integers(1 << 20)), 1, np.arange(B), cfg, window=WINDOW)
            moved.append(float((rows[:, 0] != 0).mean()))
            launches.append((torch.from_numpy(rng.integers(0, frames - WINDOW, B)).to(dev),
                             nat.augment_params(rows, B, WINDOW, dev)))
        fns = {
            "augment": lambda a: nat.gather_windows_augment(spec_tm, a[0], WINDOW, a[1], identity, mics, 0.0, out=out),
            "mic": lambda a: nat.gather_windows_mic(spec_tm, a[0], WINDOW, a[1], perm, "logmel_gcc", mics, 0.0, out=out),
        }
        runs = {k: Burst(fn, launches) for k, fn in fns.items()}
        for run in runs.values():                                  # warm up both graphs
            run.us_per_launch()
        samples = {k: [] for k in fns}
        for _ in range(bursts):                                    # alternate the two inside every round
            for k, run in runs.items():
                samples[k].append(run.us_per_launch())
        row = {"moved_share": round(statistics.mean(moved), 4)}
        for k, v in samples.items():
            med = statistics.median(v)
            row[k] = {"us_per_launch_median": round(med, 3), "us_min": round(min(v), 3), "us_max": round(max(v), 3),
                      "bytes_moved": 2 * unit, "bytes_per_s": round(2 * unit / (med * 1e-6), 0),
                      "share_of_8TBps": round(2 * unit / (med * 1e-6) / HBM_PEAK, 4)}
        row["ratio"] = round(row["mic"]["us_per_launch_median"] / row["augment"]["us_per_launch_median"], 3)
        result["cases"][case] = row
    return result


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None)
    ap.add_argument("--frames", type=int, default=120000, help="timeline length (40 min of audio: larger than the Infinity Cache)")
    ap.add_argument("--bursts", type=int, default=30)
    ap.add_argument("--burst-len", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_mic_swap.py measures on the GPU: no ROCm device visible")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    doc = {"shape": {"B": B, "window": WINDOW},
           "kernels": [bench_kernels(dev, c, pos, args.frames, args.bursts, args.burst_len) for c, pos in arrays().items()]}
    text = json.dumps(doc, indent=1)
    print(text)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
