#!/usr/bin/env python
"""Cost of the per-bin feature standardisation (csrc/standardise.hip and the affine gathers), on the GPU.

  python tools/bench_standardise.py [--out profiles/standardise.json]

(i) seld_feature_moments on a one-hour, 7-channel timeline (180 000 frames of 7 x 64 fp32 = 323 MB): device events around
each call after warm-up.  Bytes are the algorithm's: the timeline read once (the slab partials, 1.3 MB written and read once,
are counted too).  The share of peak is bytes over the 8 TB/s HBM peak over the measured time -- the pass is bound by memory.

(ii) every affine gather against the gather it extends, at the training shape (B = 32 windows of 250 frames, C = 4 and 7), the
two alternating in the same process.  A timed sample is a burst of launches captured as one HIP graph and replayed between
two device events (tools/bench_augment.py: one launch is a few microseconds), every launch with its own random starts on a
timeline larger than the Infinity Cache.  Reported: both medians, their min .. max, and whether the difference of the
medians lies inside the larger of the two spreads.
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
for p in (str(ROOT), str(ROOT / "sound-event-localization-detection_amd"), str(ROOT / "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

from bench_augment import B, WINDOW, HBM_PEAK, Burst, case_rows  # noqa: E402

J = 36


def bench_moments(dev, frames, channels, repeats):
    import seld_native as nat
    spec_tm = torch.randn(frames, channels, 64, device=dev) * 15 - 40
    slabs = -(-frames // 1024)
    nbytes = spec_tm.numel() * 4 + 2 * slabs * 2 * channels * 64 * 8
    for _ in range(3):
        first = nat.feature_moments(spec_tm)
    torch.cuda.synchronize()
    again = nat.feature_moments(spec_tm)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms = []
    for _ in range(repeats):
        e0.record()
        nat.feature_moments(spec_tm)
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    med = statistics.median(ms)
    mean = (first[0] / frames).mean().item()
    return {"frames": frames, "channels": channels, "timeline_bytes": spec_tm.numel() * 4, "bytes_moved": nbytes,
            "slabs": slabs, "repeats": repeats, "ms_median": round(med, 4), "ms_min": round(min(ms), 4),
            "ms_max": round(max(ms), 4), "bytes_per_s": round(nbytes / (med * 1e-3), 0),
            "share_of_8TBps_hbm_peak": round(nbytes / (med * 1e-3) / HBM_PEAK, 4), "bound": "memory",
            "two_calls_identical_bits": bool(torch.equal(first.view(torch.int64), again.view(torch.int64))),
            "mean_of_means": round(mean, 4)}


def bench_gathers(dev, channels, frames, bursts, burst_len):
    import seld_augment
    import seld_native as nat
    rng = np.random.default_rng(channels)
    spec_tm = torch.randn(frames, channels, 64, device=dev) * 30
    rot_tm = torch.rand(frames, 3, 64, device=dev) + 0.5
    rot_tm[:, 2] *= 0.3
    scale = (torch.rand(channels, 64, device=dev) + 0.05).contiguous()
    shift = torch.randn(channels, 64, device=dev).contiguous()
    feature_set = "logmel" if channels == 4 else "logmel_iv"
    table = seld_augment.channel_table(feature_set, channels)
    starts = [torch.from_numpy(rng.integers(0, frames - WINDOW, B)).to(dev) for _ in range(burst_len)]
    out = torch.empty(B, WINDOW, channels, 64, device=dev)
    nbytes = 2 * out.numel() * 4
    drawn = case_rows("drawn", rng)
    params = nat.augment_params(drawn, B, WINDOW, dev)
    rotated = drawn.copy()
    rotated[:, 9] = rng.integers(0, J, B)                          # most windows take the rotated path
    params_rot = nat.augment_params(rotated, B, WINDOW, dev, steps=J)
    aff = {"scale": scale, "shift": shift}
    pairs = {
        "plain": (lambda s: nat.gather_windows(spec_tm, s, WINDOW, out=out),
                  lambda s: nat.gather_windows_affine(spec_tm, s, WINDOW, scale, shift, out=out)),
        "augment": (lambda s: nat.gather_windows_augment(spec_tm, s, WINDOW, params, table, channels, 0.0, out=out),
                    lambda s: nat.gather_windows_augment(spec_tm, s, WINDOW, params, table, channels, 0.0, out=out, **aff)),
        "rotate": (lambda s: nat.gather_windows_rotate(spec_tm, rot_tm, s, WINDOW, params_rot, table, "WYZX", J, channels, 0.0,
                                                       out=out),
                   lambda s: nat.gather_windows_rotate(spec_tm, rot_tm, s, WINDOW, params_rot, table, "WYZX", J, channels, 0.0,
                                                       out=out, **aff)),
    }
    result = {"channels": channels, "timeline_frames": frames, "bytes_moved": nbytes, "table_bytes": 2 * channels * 64 * 4,
              "bursts": bursts, "launches_per_burst": burst_len, "gathers": {}}
    for name, (base_fn, affine_fn) in pairs.items():
        runs = {"base": Burst(base_fn, starts), "affine": Burst(affine_fn, starts)}
        for run in runs.values():
            run.us_per_launch()
        samples = {"base": [], "affine": []}
        for _ in range(bursts):                                    # alternate the two inside every round
            for k, run in runs.items():
                samples[k].append(run.us_per_launch())
        row = {}
        for k, v in samples.items():
            med = statistics.median(v)
            row[k] = {"us_per_launch_median": round(med, 3), "us_min": round(min(v), 3), "us_max": round(max(v), 3),
                      "bytes_per_s": round(nbytes / (med * 1e-6), 0)}
        diff = row["affine"]["us_per_launch_median"] - row["base"]["us_per_launch_median"]
        spread = max(row[k]["us_max"] - row[k]["us_min"] for k in row)
        row["affine_minus_base_us"] = round(diff, 3)
        row["spread_us"] = round(spread, 3)
        row["ratio"] = round(row["affine"]["us_per_launch_median"] / row["base"]["us_per_launch_median"], 3)
        row["difference_inside_spread"] = bool(abs(diff) <= spread)
        result["gathers"][name] = row
    return result


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None)
    ap.add_argument("--moment-frames", type=int, default=180000, help="one hour of audio at 50 frames per second")
    ap.add_argument("--moment-repeats", type=int, default=30)
    ap.add_argument("--frames", type=int, default=120000, help="timeline of the gathers (larger than the Infinity Cache)")
    ap.add_argument("--bursts", type=int, default=30)
    ap.add_argument("--burst-len", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_standardise.py measures on the GPU: no ROCm device visible")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    doc = {"shape": {"B": B, "window": WINDOW},
           "moments": bench_moments(dev, args.moment_frames, 7, args.moment_repeats),
           "gathers": [bench_gathers(dev, c, args.frames, args.bursts, args.burst_len) for c in (4, 7)]}
    text = json.dumps(doc, indent=1)
    print(text)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
