#!/usr/bin/env python
"""Cost of mixing two training windows in the device window gather (csrc/mix.hip), on the GPU.

  python tools/bench_mix.py                      kernels + end to end, one JSON document (also --out FILE)
  python tools/bench_mix.py --skip-e2e           kernels only
  rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_mix.py --profile all
                                                 a short run of its own for the profiler: the augmenting pair and the
                                                 mixing pair of ONE case (none | all | drawn), C = 4 and 7

Kernels, at the training shape (B = 32 windows of 250 frames, C_total = 4 and 7): the mixing pair (mix_chunks_kernel or
mix_units_kernel + mix_mask_kernel) against the augmenting pair (gather_augment_kernel + permute_mask_kernel<false>) on the
same starts and parameter rows, alternating in one process, measured as tools/bench_augment.py measures: a timed sample is a
burst of launches captured as one HIP graph and replayed between two device events, every launch of a burst with its own
random starts and partners, on a timeline larger than the Infinity Cache.  Cases: no window mixed (the cost of the kernel
form itself), every window mixed (identity patterns, gain 1), and the drawn case (AUGMENT_MIX_PROB 0.5, spatial patterns on
both operands, two time and two frequency masks).  Bytes are the algorithm's, counted as DESIGN.md section 11.5 counts them:
the augmenting gather moves 2 units per window (read once, written once), a mixed window 3 (two reads, one write), features
and labels alike.

End to end: full-size CRNN, batch 32, captured training steps fed by SELDDataset.device_batch, AUGMENT_MIX_PROB off and on
(0.5) in alternating rounds of the same process; the on side includes both host draws and both table uploads.
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
for p in (str(ROOT), str(ROOT / "sound-event-localization-detection_amd"), str(ROOT / "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

from bench_augment import Burst  # noqa: E402  (the captured burst of launches, shared with the augmentation's bench)

B, WINDOW, I, J = 32, 250, 18, 36
HBM_PEAK = 8.0e12
CASES = ("none", "all", "drawn")
DRAWN = dict(AUGMENT_SPATIAL=True, AUGMENT_TIME_MASKS=2, AUGMENT_TIME_MASK_MAX=40, AUGMENT_FREQ_MASKS=2, AUGMENT_FREQ_MASK_MAX=12,
             AUGMENT_MIX_PROB=0.5, AUGMENT_MIX_GAIN_DB=6.0)


def case_tables(case, rng, frames):
    """(parameter rows int32 [B, 12], partner starts, partner patterns, gains) of one launch."""
    import seld_augment
    rows = seld_augment.identity_rows(B)
    starts_b = rng.integers(0, frames - WINDOW, B)
    patterns_b, gains = np.zeros(B, dtype=np.int32), np.zeros(B, dtype=np.float32)
    if case == "all":
        gains[:] = 1.0
    elif case == "drawn":
        cfg = SimpleNamespace(**DRAWN)
        seed = int(rng.integers(1 << 20))
        rows = seld_augment.draw(seed, 1, np.arange(B), cfg, window=WINDOW)
        partner, patterns_b, gains = seld_augment.draw_mix(seed, 1, np.arange(B), cfg, frames - WINDOW)
        starts_b = np.where(partner < 0, 0, partner)               # any window start of the timeline
    return rows, starts_b, patterns_b, gains


def bench_kernels(dev, channels, frames, bursts, burst_len, only=None):
    import seld_augment
    import seld_native as nat
    rng = np.random.default_rng(channels)
    spec_tm = torch.randn(frames, channels, 64, device=dev) * 30
    mask_tm = torch.from_numpy(np.where(rng.random((frames, I * J)) < 0.03, 1 << rng.integers(0, 13, (frames, I * J)), 0)
                               .astype(np.uint16)).to(dev)
    feature_set = "logmel" if channels == 4 else "logmel_iv"
    iv = seld_augment.mix_iv_channels(feature_set, channels)
    table = seld_augment.channel_table(feature_set, channels)
    spec_out = torch.empty(B, WINDOW, channels, 64, device=dev)
    mask_out = torch.empty(B, WINDOW, I * J, dtype=torch.uint16, device=dev)
    spec_unit, mask_unit = spec_out.numel() * 4, mask_out.numel() * 2
    result = {"channels": channels, "timeline_frames": frames, "spec_bytes_per_unit": spec_unit, "label_bytes_per_unit": mask_unit,
              "bursts": bursts, "launches_per_burst": burst_len, "cases": {}}
    for case in CASES if only is None else (only,):
        launches, share = [], []
        for _ in range(burst_len):                                 # every launch of a burst: its own starts, rows and partners
            rows, starts_b, patterns_b, gains = case_tables(case, rng, frames)
            share.append(float((gains > 0).mean()))
            launches.append((torch.from_numpy(rng.integers(0, frames - WINDOW, B)).to(dev),
                             nat.augment_params(rows, B, WINDOW, dev), nat.mix_partners(starts_b, patterns_b, gains, dev)))
        mixed_share = statistics.mean(share)
        fns = {
            "augment_spec": lambda a: nat.gather_windows_augment(spec_tm, a[0], WINDOW, a[1], table, channels, 0.0, out=spec_out),
            "mix_spec": lambda a: nat.gather_windows_mix(spec_tm, a[0], WINDOW, a[1], a[2], table, channels, 0.0, iv, out=spec_out),
            "augment_labels": lambda a: nat.gather_windows_permute(mask_tm, a[0], WINDOW, a[1], I, J, out=mask_out),
            "mix_labels": lambda a: nat.gather_windows_mix_mask(mask_tm, a[0], WINDOW, a[1], a[2], I, J, out=mask_out),
        }
        runs = {k: Burst(fn, launches) for k, fn in fns.items()}
        for run in runs.values():                                  # warm up every graph
            run.us_per_launch()
        samples = {k: [] for k in fns}
        for _ in range(bursts):                                    # alternate the four inside every round
            for k, run in runs.items():
                samples[k].append(run.us_per_launch())
        row = {"mixed_share": round(mixed_share, 4), "byte_ratio": round((2.0 + mixed_share) / 2.0, 4)}
        for k, v in samples.items():
            med = statistics.median(v)
            units = 2.0 + (mixed_share if k.startswith("mix") else 0.0)
            nbytes = units * (spec_unit if k.endswith("spec") else mask_unit)
            row[k] = {"us_per_launch_median": round(med, 3), "us_min": round(min(v), 3), "us_max": round(max(v), 3),
                      "bytes_moved": int(nbytes), "bytes_per_s": round(nbytes / (med * 1e-6), 0),
                      "share_of_8TBps": round(nbytes / (med * 1e-6) / HBM_PEAK, 4)}
        aug = row["augment_spec"]["us_per_launch_median"] + row["augment_labels"]["us_per_launch_median"]
        mix = row["mix_spec"]["us_per_launch_median"] + row["mix_labels"]["us_per_launch_median"]
        row["ratio_spec"] = round(row["mix_spec"]["us_per_launch_median"] / row["augment_spec"]["us_per_launch_median"], 3)
        row["ratio_labels"] = round(row["mix_labels"]["us_per_launch_median"] / row["augment_labels"]["us_per_launch_median"], 3)
        row["ratio_pair"] = round(mix / aug, 3)
        result["cases"][case] = row
    return result


def bench_end_to_end(dev, rounds, steps, features):
    """Captured CRNN bs-32 training steps, AUGMENT_MIX_PROB off / on (0.5) in alternating rounds."""
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
        mix_cfg = SimpleNamespace(AUGMENT_MIX_PROB=0.5, AUGMENT_MIX_GAIN_DB=6.0)
        order = np.random.default_rng(1).permutation(len(ds))

        def run(on, epoch):
            static = getattr(stepper, "static_inputs", None)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for n in range(steps):
                idx = order[(n * B) % (len(ds) - B):][:B]
                if on:
                    params = seld_augment.draw(3, epoch, idx, mix_cfg, window=WINDOW)
                    mix = seld_augment.draw_mix(3, epoch, idx, mix_cfg, len(ds))
                    spec, mask = ds.device_batch(idx, out=static, augment=params, mix=mix)
                else:
                    spec, mask = ds.device_batch(idx, out=static)
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
                "windows": len(ds), "rounds": rounds, "steps_per_round": steps, "mix_prob": 0.5,
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
    ap.add_argument("--e2e-features", default="logmel_iv", choices=("logmel", "logmel_iv"))
    ap.add_argument("--profile", default=None, choices=CASES, help="short run of one case at C = 4 and 7 for rocprofv3")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_mix.py measures on the GPU: no ROCm device visible")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    if args.profile:
        doc = {"profile_case": args.profile,
               "kernels": [bench_kernels(dev, c, args.frames, 5, args.burst_len, only=args.profile) for c in (4, 7)]}
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
