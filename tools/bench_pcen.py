#!/usr/bin/env python
"""Cost of the per-channel energy normalisation (csrc/pcen.hip), on the GPU.

  python tools/bench_pcen.py [--out profiles/pcen.json]

(i) seld_pcen on one hour of 7-channel features (one clip of 180 000 frames, C_log = 4) and on 60 clips of 60 s (3 000 frames
each): device events around each call after warm-up, out of place into a buffer allocated once, in place, and out of place
with a 1 GiB buffer overwritten before every timed call (the input then comes from HBM, not from the Infinity Cache: what the
once-per-recording call sees).  Bytes are the
algorithm's: the log-mel channels read by both launches and written once, the workspace written once and read once per
use as HBM traffic; the Horner reads of the chunk carries beyond the first (served by the caches: the whole workspace is
0.7 MB) are reported apart.  The share of peak is those bytes over the 8 TB/s HBM peak over the measured time.  The moments
kernel of csrc/standardise.hip is timed on the same hour-long timeline in the same process, for the comparison.

(ii) the wall time of a dataset construction (SELDDataset.from_pcm, 'logmel_iv', clips of 60 s) with and without Config.PCEN,
the two alternating in the same process, a device synchronise inside the host clock.
"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
for p in (str(ROOT), str(ROOT / "sound-event-localization-detection_amd"), str(ROOT / "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

HBM_PEAK = 8.0e12
CHUNK = 256
SETTING = dict(tau=0.4, alpha=0.98, delta=2.0, r=0.5, eps=1e-10)


def _summary(ms):
    return {"ms_median": round(statistics.median(ms), 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4)}


def _time(fn, repeats, flush=None):
    """Device-event times of ``repeats`` calls; ``flush``: a buffer larger than the caches, overwritten before every timed
    call so that the call reads its input from HBM (what the once-per-recording call sees)."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms = []
    for i in range(repeats):
        if flush is not None:
            flush.fill_(float(i))
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return ms


def bench_kernel(dev, clips, frames, channels, c_log, repeats, with_moments):
    import seld_native as nat
    x = torch.randn(clips, frames, channels, 64, device=dev) * 15 - 40
    x[:, :, :c_log].clamp_(min=-100.0)
    keep = x.clone()
    out = torch.empty_like(x)
    s = nat.pcen_coefficient(SETTING["tau"])
    args = (c_log, s, SETTING["alpha"], SETTING["delta"], SETTING["r"], SETTING["eps"])
    chunks = -(-frames // CHUNK)
    logmel_bytes = clips * frames * c_log * 64 * 4
    workspace_bytes = clips * chunks * c_log * 64 * 4
    carry_reads = clips * (chunks * (chunks - 1) // 2 + chunks) * c_log * 64 * 4    # Horner: chunk k reads E[0] and k aggregates
    hbm_bytes = 3 * logmel_bytes + 2 * workspace_bytes
    for _ in range(3):
        nat.pcen(x, *args, out=out)
    torch.cuda.synchronize()
    first = out.clone()
    oop = _time(lambda: nat.pcen(x, *args, out=out), repeats)
    same = bool(torch.equal(first.view(torch.int32)[:, :, :c_log], out.view(torch.int32)[:, :, :c_log]))
    nat.pcen(x, *args, out=x)                                   # in place: the values change from call to call, the work does not
    torch.cuda.synchronize()
    in_place_equal = bool(torch.equal(x.view(torch.int32)[:, :, :c_log], first.view(torch.int32)[:, :, :c_log]))
    x.copy_(keep)
    inp = _time(lambda: nat.pcen(x, *args, out=x), repeats)
    x.copy_(keep)
    flush = torch.empty(1 << 28, dtype=torch.float32, device=dev)            # 1 GiB: four times the Infinity Cache
    cold = _time(lambda: nat.pcen(x, *args, out=out), repeats, flush=flush)
    del flush
    row = {"clips": clips, "frames": frames, "channels": channels, "c_log": c_log, "chunks_per_clip": chunks,
           "logmel_bytes": logmel_bytes, "workspace_bytes": workspace_bytes, "hbm_bytes_moved": hbm_bytes,
           "carry_bytes_read_through_caches": carry_reads, "repeats": repeats, "setting": SETTING,
           "out_of_place": _summary(oop), "in_place": _summary(inp), "out_of_place_1GiB_overwritten_first": _summary(cold),
           "two_calls_identical_bits": same, "in_place_equals_out_of_place_bits": in_place_equal, "bound": "memory"}
    for key in ("out_of_place", "in_place", "out_of_place_1GiB_overwritten_first"):
        med = row[key]["ms_median"]
        row[key]["bytes_per_s"] = round(hbm_bytes / (med * 1e-3), 0)
        row[key]["share_of_8TBps_hbm_peak"] = round(hbm_bytes / (med * 1e-3) / HBM_PEAK, 4)
    if with_moments:
        x.copy_(keep)
        timeline = x.view(clips * frames, channels, 64)
        for _ in range(3):
            nat.feature_moments(timeline)
        torch.cuda.synchronize()
        ms = _time(lambda: nat.feature_moments(timeline), repeats)
        nbytes = timeline.numel() * 4 + 2 * (-(-clips * frames // 1024)) * 2 * channels * 64 * 8
        row["moments_same_timeline"] = dict(_summary(ms), bytes_moved=nbytes,
                                            share_of_8TBps_hbm_peak=round(nbytes / (statistics.median(ms) * 1e-3) / HBM_PEAK, 4))
    return row


def bench_dataset(dev, n_clips, seconds, rounds):
    import dataset
    from config import Config
    gen = torch.Generator().manual_seed(0)
    clips = [(torch.randn(4, 24000 * seconds, generator=gen) * 0.1).to(dev) for _ in range(n_clips)]
    rows = [[[0, 0, 0, 10, 0]] for _ in range(n_clips)]
    saved = (Config.FEATURE_SET, Config.PCEN)
    Config.FEATURE_SET = "logmel_iv"
    times = {"off": [], "on": []}
    try:
        for r in range(rounds + 1):                              # round 0 warms both paths up
            for key in ("off", "on"):
                Config.PCEN = key == "on"
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                ds = dataset.SELDDataset.from_pcm(clips, rows, device=dev)
                torch.cuda.synchronize()
                if r:
                    times[key].append((time.perf_counter() - t0) * 1e3)
                frames = ds.total_frames
                del ds
    finally:
        Config.FEATURE_SET, Config.PCEN = saved
    doc = {"clips": n_clips, "seconds_each": seconds, "timeline_frames": frames, "feature_set": "logmel_iv", "rounds": rounds}
    for key, v in times.items():
        doc[key] = _summary(v)
    doc["on_minus_off_ms"] = round(doc["on"]["ms_median"] - doc["off"]["ms_median"], 3)
    doc["spread_ms"] = round(max(doc[k]["ms_max"] - doc[k]["ms_min"] for k in ("off", "on")), 3)
    return doc


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--hour-frames", type=int, default=180000, help="one hour of audio at 50 frames per second")
    ap.add_argument("--clips", type=int, default=60)
    ap.add_argument("--clip-frames", type=int, default=3000, help="60 s at 50 frames per second")
    ap.add_argument("--dataset-clips", type=int, default=8)
    ap.add_argument("--dataset-rounds", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_pcen.py measures on the GPU: no ROCm device visible")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    doc = {"hour": bench_kernel(dev, 1, args.hour_frames, 7, 4, args.repeats, with_moments=True),
           "clips": bench_kernel(dev, args.clips, args.clip_frames, 7, 4, args.repeats, with_moments=False),
           "dataset_construction": bench_dataset(dev, args.dataset_clips, 60, args.dataset_rounds)}
    text = json.dumps(doc, indent=1)
    print(text)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
