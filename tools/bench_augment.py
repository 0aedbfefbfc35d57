#!/usr/bin/env python
"""Cost of the training augmentation in the device window gather (csrc/augment.hip), on the GPU.

  python tools/bench_augment.py                      kernels + end to end, one JSON document (also --out FILE)
  python tools/bench_augment.py --skip-e2e           kernels only
  rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_augment.py --profile mirror
                                                     a short run of its own for the profiler: the plain pair and the
                                                     augmented pair of ONE case (identity | rotation | mirror | drawn), C = 4

Kernels, at the training shape (B = 32 windows of 250 frames, C_total = 4 and 7): the augmented pair (gather_augment_kernel +
permute_mask_kernel<false>) against the plain pair (gather_rows_kernel twice) on the same starts, alternating in one process.  A
timed sample is a burst of launches captured as one HIP graph and replayed between two device events (one launch is a few
microseconds: less than a Python launch costs the host), every launch of a burst with its own random starts; the timeline is
larger than the Infinity Cache, so the reads come from HBM as they do in an epoch over hours of audio.  Bytes are the algorithm's: every output byte written once and read
once from the timeline.  A burst's time includes the launch boundaries between its kernels, the same for both sides; kernel
times proper come from the profiler run.

End to end: full-size CRNN, batch 32, captured training steps fed by SELDDataset.device_batch, augmentation off and on in
alternating rounds of the same process; the on side includes the host draw and the parameter upload.
"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
for p in (str(ROOT), str(ROOT / "sound-event-localization-detection_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

B, WINDOW, I, J = 32, 250, 18, 36
HBM_PEAK = 8.0e12
CASES = ("identity", "rotation", "mirror", "drawn")


def case_rows(case, rng):
    import seld_augment
    rows = seld_augment.identity_rows(B)
    if case == "rotation":
        rows[:, 0] = 2
    elif case == "mirror":
        rows[:, 0] = 8
    elif case == "drawn":                      # what training draws: uniform pattern, two time and two frequency masks
        cfg = SimpleNamespace(AUGMENT_SPATIAL=True, AUGMENT_TIME_MASKS=2, AUGMENT_TIME_MASK_MAX=40, AUGMENT_FREQ_MASKS=2,
                              AUGMENT_FREQ_MASK_MAX=12)
        rows = seld_augment.draw(int(rng.integers(1 << 20)), 1, np.arange(B), cfg, window=WINDOW)
    return rows


class Burst:
    """len(starts) launches of fn(starts[i]) captured as one HIP graph: replayed, the kernels run back to back on the device
    (a Python launch costs more host time than one of these kernels runs, so an eager loop would time the host)."""

    def __init__(self, fn, starts):
        self.n = len(starts)
        for s in starts[:2]:                                       # load the code object before capturing
            fn(s)
        torch.cuda.synchronize()
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            for s in starts:
                fn(s)
        self.e0, self.e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def us_per_launch(self):
        self.e0.record()
        self.graph.replay()
        self.e1.record()
        self.e1.synchronize()
        return self.e0.elapsed_time(self.e1) * 1e3 / self.n


def bench_kernels(dev, channels, frames, bursts, burst_len, only=None):
    import seld_augment
    import seld_native as nat
    rng = np.random.default_rng(channels)
    spec_tm = torch.randn(frames, channels, 64, device=dev) * 30
    mask_tm = torch.from_numpy(np.where(rng.random((frames, I * J)) < 0.03, 1 << rng.integers(0, 13, (frames, I * J)), 0)
                               .astype(np.uint16)).to(dev)
    feature_set = "logmel" if channels == 4 else "logmel_iv"
    table = seld_augment.channel_table(feature_set, channels)
    starts = [torch.from_numpy(rng.integers(0, frames - WINDOW, B)).to(dev) for _ in range(burst_len)]
    spec_out = torch.empty(B, WINDOW, channels, 64, device=dev)
    mask_out = torch.empty(B, WINDOW, I * J, dtype=torch.uint16, device=dev)
    spec_bytes, mask_bytes = 2 * spec_out.numel() * 4, 2 * mask_out.numel() * 2
    result = {"channels": channels, "timeline_frames": frames, "spec_bytes_moved": spec_bytes, "label_bytes_moved": mask_bytes,
              "bursts": bursts, "launches_per_burst": burst_len, "cases": {}}
    for case in CASES if only is None else (only,):
        params = nat.augment_params(case_rows(case, rng), B, WINDOW, dev)
        fns = {
            "plain_spec": lambda s: nat.gather_windows(spec_tm, s, WINDOW, out=spec_out),
            "augment_spec": lambda s: nat.gather_windows_augment(spec_tm, s, WINDOW, params, table, channels, 0.0, out=spec_out),
            "plain_labels": lambda s: nat.gather_windows(mask_tm, s, WINDOW, out=mask_out),
            "augment_labels": lambda s: nat.gather_windows_permute(mask_tm, s, WINDOW, params, I, J, out=mask_out),
        }
        runs = {k: Burst(fn, starts) for k, fn in fns.items()}
        for run in runs.values():                                  # warm up every graph
            run.us_per_launch()
        samples = {k: [] for k in fns}
        for _ in range(bursts):                                    # alternate the four inside every round
            for k, run in runs.items():
                samples[k].append(run.us_per_launch())
        row = {}
        for k, v in samples.items():
            med = statistics.median(v)
            nbytes = spec_bytes if k.endswith("spec") else mask_bytes
            row[k] = {"us_per_launch_median": round(med, 3), "us_min": round(min(v), 3), "us_max": round(max(v), 3),
                      "bytes_per_s": round(nbytes / (med * 1e-6), 0), "share_of_8TBps": round(nbytes / (med * 1e-6) / HBM_PEAK, 4)}
        plain = row["plain_spec"]["us_per_launch_median"] + row["plain_labels"]["us_per_launch_median"]
        aug = row["augment_spec"]["us_per_launch_median"] + row["augment_labels"]["us_per_launch_median"]
        row["ratio_spec"] = round(row["augment_spec"]["us_per_launch_median"] / row["plain_spec"]["us_per_launch_median"], 3)
        row["ratio_labels"] = round(row["augment_labels"]["us_per_launch_median"] / row["plain_labels"]["us_per_launch_median"], 3)
        row["ratio_pair"] = round(aug / plain, 3)
        result["cases"][case] = row
    return result


def bench_end_to_end(dev, rounds, steps, features):
    """Captured CRNN bs-32 training steps, augmentation off / on in alternating rounds."""
    import dataset
    import seld_augment
    import trainer
    from config import Config
    cfg = trainer.config
    saved = Config.FEATURE_SET
    Config.FEATURE_SET = features
    try:
        cfg.MODEL_TYPE, cfg.BATCH_SIZE = "crnn", B
        torch.manual_seed(0)
        rng = np.random.default_rng(0)
        clips = [(torch.randn(4, 24000 * 60, device=dev) * 0.1) for _ in range(4)]
        rows = []
        for _ in clips:
            t = np.repeat(np.arange(600), 2)
            rows.append(np.stack([t, rng.integers(0, 13, t.size), np.tile([0, 1], 600), rng.integers(-179, 180, t.size),
                                  rng.integers(-89, 90, t.size)], axis=1).astype(np.int64))
        ds = dataset.SELDDataset.from_pcm(clips, rows, device=dev)
        model = trainer.prepare_model_for_device(trainer.build_model((ds.I, ds.J), n_channels=ds.n_channels), dev).train()
        trainer.enable_master_weights(model, dev)
        graphed = trainer.graph_step_enabled(dev, 1)
        weights = torch.ones(14, device=dev)
        weights[13] = 0.05
        crit = trainer.SMRSELDLoss(loss_type="mse", w_class=1.0, grid_size=(ds.I, ds.J), class_weights=weights)
        opt = trainer.make_optimizer(model, cfg.LEARNING_RATE, dev, capturable=graphed)
        stepper = trainer.make_stepper(model, crit, opt, dev, 1)
        aug_cfg = SimpleNamespace(AUGMENT_SPATIAL=True, AUGMENT_TIME_MASKS=2, AUGMENT_TIME_MASK_MAX=40, AUGMENT_FREQ_MASKS=2,
                                  AUGMENT_FREQ_MASK_MAX=12)
        order = np.random.default_rng(1).permutation(len(ds))

        def run(on, epoch):
            static = getattr(stepper, "static_inputs", None)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for n in range(steps):
                idx = order[(n * B) % (len(ds) - B):][:B]
                params = seld_augment.draw(3, epoch, idx, aug_cfg, window=WINDOW) if on else None
                spec, mask = ds.device_batch(idx, out=static, augment=params)
                stepper(spec, mask)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3 / steps

        for on in (False, True, False, True):                       # capture + warm both paths
            run(on, 0)
        off, onn = [], []
        for r in range(rounds):
            off.append(run(False, r + 1))
            onn.append(run(True, r + 1))
        if hasattr(stepper, "close"):
            stepper.close()
        med_off, med_on = statistics.median(off), statistics.median(onn)
        spread = max(max(off) - min(off), max(onn) - min(onn))
        return {"model": "crnn", "batch": B, "features": features, "channels": ds.n_channels, "graph_step": bool(graphed),
                "windows": len(ds), "rounds": rounds, "steps_per_round": steps,
                "ms_per_step_off": [round(v, 4) for v in off], "ms_per_step_on": [round(v, 4) for v in onn],
                "median_off_ms": round(med_off, 4), "median_on_ms": round(med_on, 4), "on_minus_off_ms": round(med_on - med_off, 4),
                "spread_ms": round(spread, 4), "difference_inside_spread": bool(abs(med_on - med_off) <= spread)}
    finally:
        Config.FEATURE_SET = saved


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None)
    ap.add_argument("--frames", type=int, default=120000, help="timeline length (40 min of audio: larger than the Infinity Cache)")
    ap.add_argument("--bursts", type=int, default=30)
    ap.add_argument("--burst-len", type=int, default=20)
    ap.add_argument("--skip-e2e", action="store_true")
    ap.add_argument("--e2e-rounds", type=int, default=8)
    ap.add_argument("--e2e-steps", type=int, default=12)
    ap.add_argument("--e2e-features", default="logmel", choices=("logmel", "logmel_iv"))
    ap.add_argument("--profile", default=None, choices=CASES, help="short run of one case at C = 4 for rocprofv3")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_augment.py measures on the GPU: no ROCm device visible")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    if args.profile:
        doc = {"profile_case": args.profile, "kernels": [bench_kernels(dev, 4, args.frames, 5, args.burst_len, only=args.profile)]}
    else:
        doc = {"shape": {"B": B, "window": WINDOW, "grid": [I, J]},
               "kernels": [bench_kernels(dev, c, args.frames, args.bursts, args.burst_len) for c in (4, 7)]}
        doc["end_to_end"] = None if args.skip_e2e else bench_end_to_end(dev, args.e2e_rounds, args.e2e_steps, args.e2e_features)
    text = json.dumps(doc, indent=1)
    print(text)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
