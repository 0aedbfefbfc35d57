#!/usr/bin/env python
"""Cost of the per-window class statistics behind class-balanced window sampling (csrc/balance.hip),
on the GPU.

  python tools/bench_balance.py [--out profiles/balance.json]

(i) seld_frame_class_mask and seld_window_class_frames on a one-hour label timeline (180 000 frames x 648 cells of uint16 =
233 MB) and on a ten-hour one (2.33 GB): device events around each call after warm-up.  Bytes are the algorithm's: the
frame pass reads the timeline once and writes 2 B per frame; the window pass reads 2 B per frame and window (500 B per
window of 250 frames) and writes 64 B per window.  The share of peak is bytes over the 8 TB/s HBM peak over the measured
time: the frame pass is bound by memory.  The one-hour timeline is SMALLER than the 256 MiB Infinity Cache, so calls
repeated back to back read it from there; `cold` samples overwrite a 1 GiB buffer before every timed call, which is what
the once-per-run call sees.  The ten-hour timeline does not fit either way.

(ii) seld_feature_moments -- the project's other once-per-run reduction over a timeline -- on the same number of frames of
7-channel features (323 MB per hour), timed the same way.

(iii) the exposure report (seld_balance.exposure) of the benchmark's synthetic labels (bench.synth_metadata, 40 clips of
60 s) and of a skewed synthetic timeline (sparse events, class frequencies 1 : 2 : 4 : ...), each with the default settings.
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

HBM_PEAK = 8.0e12
CELLS, WINDOW, HOP, CLASSES = 648, 250, 50, 14


def _timed(fn, repeats, evict=None):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms = []
    for _ in range(repeats):
        if evict is not None:
            evict.fill_(1)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return ms


def _row(ms, nbytes):
    med = statistics.median(ms)
    return {"ms_median": round(med, 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4),
            "bytes_per_s": round(nbytes / (med * 1e-3), 0), "share_of_8TBps_hbm_peak": round(nbytes / (med * 1e-3) / HBM_PEAK, 4)}


def sparse_timeline(dev, frames, seed=0):
    """uint16 [frames, 648] on the device: ~0.3 % of the cells of ~60 % of the frames hold one of 13 classes."""
    g = torch.Generator(device=dev).manual_seed(seed)
    mask = torch.zeros((frames, CELLS), dtype=torch.int16, device=dev)
    step = 20000
    for lo in range(0, frames, step):
        n = min(step, frames - lo)
        hit = torch.rand((n, CELLS), generator=g, device=dev) < 0.003
        live = torch.rand((n, 1), generator=g, device=dev) < 0.6
        bits = torch.randint(0, 13, (n, CELLS), generator=g, device=dev)
        mask[lo:lo + n] = torch.where(hit & live, torch.ones_like(bits) << bits, torch.zeros_like(bits)).to(torch.int16)
    return mask.view(torch.uint16)


def bench_counts(dev, frames, repeats, evict):
    import seld_native as nat
    mask_tm = sparse_timeline(dev, frames)
    n_windows = -(-frames // HOP)
    frame_bytes = mask_tm.numel() * 2 + frames * 2
    window_bytes = sum(min(WINDOW, frames - w * HOP) for w in range(n_windows)) * 2 + n_windows * 64
    for _ in range(3):
        rows = nat.frame_class_mask(mask_tm)
        counts = nat.window_class_frames(rows, WINDOW, HOP, n_windows, CLASSES)
    torch.cuda.synchronize()
    doc = {"frames": frames, "hours": round(frames / 180000, 2), "timeline_bytes": mask_tm.numel() * 2, "windows": n_windows,
           "repeats": repeats, "frame_pass_bytes": frame_bytes, "window_pass_bytes": window_bytes,
           "frame_pass": _row(_timed(lambda: nat.frame_class_mask(mask_tm), repeats), frame_bytes),
           "window_pass": _row(_timed(lambda: nat.window_class_frames(rows, WINDOW, HOP, n_windows, CLASSES), repeats),
                               window_bytes)}
    if evict is not None:
        doc["frame_pass_cold"] = _row(_timed(lambda: nat.frame_class_mask(mask_tm), repeats, evict), frame_bytes)
    again = nat.window_class_frames(nat.frame_class_mask(mask_tm), WINDOW, HOP, n_windows, CLASSES)
    doc["two_calls_identical"] = bool(torch.equal(counts, again))
    doc["frames_with_a_class"] = int((rows.view(torch.int16) != 0).sum())
    del mask_tm
    return doc


def bench_moments(dev, frames, channels, repeats, evict):
    import seld_native as nat
    spec_tm = torch.empty(frames, channels, 64, device=dev)
    for lo in range(0, frames, 20000):
        spec_tm[lo:lo + 20000].normal_(-40.0, 15.0)
    nbytes = spec_tm.numel() * 4 + 2 * (-(-frames // 1024)) * 2 * channels * 64 * 8
    for _ in range(3):
        nat.feature_moments(spec_tm)
    torch.cuda.synchronize()
    doc = {"frames": frames, "channels": channels, "timeline_bytes": spec_tm.numel() * 4, "bytes_moved": nbytes,
           "repeats": repeats}
    doc.update(_row(_timed(lambda: nat.feature_moments(spec_tm), repeats), nbytes))
    if evict is not None:
        doc["cold"] = _row(_timed(lambda: nat.feature_moments(spec_tm), repeats, evict), nbytes)
    return doc


def skewed_rows(clip, meta_frames=600):
    """Sparse STARSS-like rows: events of 0.5 - 4 s with gaps of 0 - 8 s, class c drawn with weight 2^-c (c = 0..7)."""
    rng = np.random.default_rng(77 + clip)
    p = 2.0 ** -np.arange(8)
    rows, t = [], int(rng.integers(0, 40))
    while t < meta_frames:
        cls, length = int(rng.choice(8, p=p / p.sum())), int(rng.integers(5, 41))
        az, el = int(rng.integers(-180, 181)), int(rng.integers(-60, 61))
        rows += [(u, cls, 0, az, el) for u in range(t, min(t + length, meta_frames))]
        t += length + int(rng.integers(0, 81))
    return np.asarray(rows, dtype=np.int64).reshape(-1, 5)


def exposure_of(dev, clips_rows, label):
    import seld_balance
    import seld_native as nat
    from config import Config
    masks = [nat.rasterise_labels(torch.from_numpy(np.ascontiguousarray(r)), 3000, device=dev) for r in clips_rows]
    mask_tm = torch.cat(masks, dim=0).contiguous()
    n_windows = -(-mask_tm.shape[0] // HOP)
    counts = nat.window_class_frames(nat.frame_class_mask(mask_tm), WINDOW, HOP, n_windows, CLASSES).cpu().numpy()
    s = seld_balance.settings(Config)
    k = seld_balance.window_weights(counts, s)
    e = seld_balance.exposure(counts, k, s)
    line = seld_balance.describe(e)
    print(f"{label}: {line}", file=sys.stderr)
    return {"labels": label, "clips": len(clips_rows), "frames": int(mask_tm.shape[0]), "settings": s, "log_line": line,
            "class_windows": e["class_windows"].tolist(), "natural": [round(float(v), 4) for v in e["natural"]],
            "expected": [round(float(v), 4) for v in e["expected"]], "silent_natural": round(e["silent_natural"], 4),
            "silent_expected": round(e["silent_expected"], 4), "distinct_weights": len(set(k.tolist()))}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None)
    ap.add_argument("--frames", type=int, default=180000, help="one hour of audio at 50 frames per second")
    ap.add_argument("--long-factor", type=int, default=10, help="the second timeline: this many times --frames")
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--evict-bytes", type=int, default=1 << 30)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_balance.py measures on the GPU: no ROCm device visible")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    import bench
    evict = torch.empty(args.evict_bytes, dtype=torch.uint8, device=dev)
    doc = {"shape": {"cells": CELLS, "window": WINDOW, "hop": HOP, "num_classes": CLASSES},
           "counts": [bench_counts(dev, args.frames, args.repeats, evict),
                      bench_counts(dev, args.frames * args.long_factor, args.repeats, None)],
           "moments": [bench_moments(dev, args.frames, 7, args.repeats, evict),
                       bench_moments(dev, args.frames * args.long_factor, 7, args.repeats, None)],
           "exposure": [exposure_of(dev, [bench.synth_metadata(i, meta_frames=600) for i in range(40)],
                                    "benchmark synthetic labels (bench.synth_metadata)"),
                        exposure_of(dev, [skewed_rows(i) for i in range(40)], "skewed synthetic labels")]}
    text = json.dumps(doc, indent=1)
    print(text)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
