#!/usr/bin/env python
"""Cost of the in-place spectral stage -- frequency shift, gain curve, cutouts -- on a gathered batch (csrc/spectral.hip;
DESIGN.md section 26), on the GPU.

  python tools/bench_spectral.py                 kernels + end to end, one JSON document (also --out FILE)
  python tools/bench_spectral.py --skip-e2e      kernels only
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_spectral.py --profile all --skip-e2e
                                                 a short run of its own for the profiler: the augmenting gather and the stage
                                                 of ONE case (none | all), C = 4, 7 and 36

Kernels, at the training shape (B = 32 windows of 250 frames, C = 4, 7 and 36): the stage against the augmenting feature
gather (gather_augment_kernel) on the same starts and the same parameter rows, alternating in one process, measured as
tools/bench_augment.py measures: a timed sample is a burst of launches captured as one HIP graph and replayed between two
device events, on a timeline larger than the Infinity Cache.  Every launch of a burst has its own starts, rows, curves and
-- the stage works in place -- its own batch buffer, so a burst's buffers do not fit the caches either.  Cases: every window
drawn (a shift, a curve, two cutouts, two time and two frequency masks) and no window drawn (identity rows: the fast path,
which neither reads nor writes the batch).  Bytes are the algorithm's, counted as DESIGN.md section 11.5 counts them: the
gather and the stage with every window drawn both move 2 units (the batch read once and written once), the fast path 0.

End to end: full-size CRNN, 'logmel_iv', batch 32, captured training steps fed by SELDDataset.device_batch, the spectral
switches off and on in alternating rounds of the same process; the on side includes the host draw and the two table uploads.
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

B, WINDOW = 32, 250
HBM_PEAK = 8.0e12
CASES = ("none", "all")
SETS = {4: ("logmel", 4, 4), 7: ("logmel_iv", 4, 7), 36: ("logmel_gcc", 8, 8)}      # feature set, log-mel, mel-axis channels
MASKS = dict(AUGMENT_TIME_MASKS=2, AUGMENT_TIME_MASK_MAX=40, AUGMENT_FREQ_MASKS=2, AUGMENT_FREQ_MASK_MAX=12)
DRAWN = dict(AUGMENT_FREQ_SHIFT_MAX=8, AUGMENT_LEVEL_DB=6.0, AUGMENT_FILTER_PROB=1.0, AUGMENT_FILTER_DB=6.0,
             AUGMENT_FILTER_BANDS=(3, 6), AUGMENT_FILTER_TYPE="linear", AUGMENT_CUTOUTS=2, AUGMENT_CUTOUT_TIME_MAX=40,
             AUGMENT_CUTOUT_FREQ_MAX=12)


def case_tables(case, rng):
    """(parameter rows int32 [B, 12], spectral rows int32 [B, 12], curves float32 [B, 64] or None) of one launch."""
    import seld_augment
    if case == "none":
        return seld_augment.identity_rows(B), seld_augment.identity_spectral_rows(B), None
    cfg = SimpleNamespace(**MASKS, **DRAWN)
    seed = int(rng.integers(1 << 20))
    rows = seld_augment.draw(seed, 1, np.arange(B), cfg, window=WINDOW)
    spectral, curves = seld_augment.draw_spectral(seed, 1, np.arange(B), cfg, window=WINDOW)
    spectral[spectral[:, 0] == 0, 0] = 1                            # every window shifted: the case's name is meant
    return rows, spectral, curves


def bench_kernels(dev, channels, frames, bursts, burst_len, only=None):
    import seld_augment
    import seld_native as nat
    rng = np.random.default_rng(channels)
    feature_set, logmel, freq = SETS[channels]
    spec_tm = torch.randn(frames, channels, 64, device=dev) * 30
    table = seld_augment.channel_table(feature_set, channels)
    unit = B * WINDOW * channels * 64 * 4
    result = {"channels": channels, "feature_set": feature_set, "timeline_frames": frames, "bytes_per_unit": unit,
              "bursts": bursts, "launches_per_burst": burst_len, "batch_buffers_bytes": unit * burst_len, "cases": {}}
    buffers = [torch.empty(B, WINDOW, channels, 64, device=dev) for _ in range(burst_len)]
    for case in CASES if only is None else (only,):
        launches = []
        for n in range(burst_len):                                  # every launch: its own starts, rows, curves and buffer
            rows, spectral, curves = case_tables(case, rng)
            starts = torch.from_numpy(rng.integers(0, frames - WINDOW, B)).to(dev)
            launches.append((starts, nat.augment_params(rows, B, WINDOW, dev), nat.spectral_params(spectral, curves, B, WINDOW, dev),
                             buffers[n]))
            nat.gather_windows(spec_tm, starts, WINDOW, out=buffers[n])              # real features under the stage
        fns = {
            "augment_gather": lambda a: nat.gather_windows_augment(spec_tm, a[0], WINDOW, a[1], table, freq, 0.0, out=buffers[0]),
            "stage": lambda a: nat.window_spectral(a[3], a[0], frames, a[1], a[2][0], a[2][1], logmel, freq, 0.0),
        }
        runs = {k: Burst(fn, launches) for k, fn in fns.items()}
        for run in runs.values():                                   # warm up both graphs
            run.us_per_launch()
        samples = {k: [] for k in fns}
        for _ in range(bursts):                                     # alternate the two inside every round
            for k, run in runs.items():
                samples[k].append(run.us_per_launch())
        row = {}
        for k, v in samples.items():
            med = statistics.median(v)
            nbytes = 0 if (k == "stage" and case == "none") else 2 * unit
            row[k] = {"us_per_launch_median": round(med, 3), "us_min": round(min(v), 3), "us_max": round(max(v), 3),
                      "bytes_moved": int(nbytes), "bytes_per_s": round(nbytes / (med * 1e-6), 0),
                      "share_of_8TBps": round(nbytes / (med * 1e-6) / HBM_PEAK, 4)}
        row["ratio_stage_to_gather"] = round(row["stage"]["us_per_launch_median"] / row["augment_gather"]["us_per_launch_median"], 3)
        row["inside_1.5x"] = bool(row["ratio_stage_to_gather"] <= 1.5)
        result["cases"][case] = row
    return result


def bench_end_to_end(dev, rounds, steps):
    """Captured CRNN bs-32 training steps on 'logmel_iv', the spectral switches off / on in alternating rounds."""
    import dataset
    import seld_augment
    import trainer
    from config import Config
    cfg = trainer.config
    saved = Config.FEATURE_SET
    Config.FEATURE_SET = "logmel_iv"
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
        on_cfg = SimpleNamespace(**dict(DRAWN, AUGMENT_FILTER_PROB=0.5))
        order = np.random.default_rng(1).permutation(len(ds))

        def run(on, epoch):
            static = getattr(stepper, "static_inputs", None)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for n in range(steps):
                idx = order[(n * B) % (len(ds) - B):][:B]
                if on:
                    spectral = seld_augment.draw_spectral(3, epoch, idx, on_cfg, window=WINDOW)
                    spec, mask = ds.device_batch(idx, out=static, spectral=spectral)
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
        return {"model": "crnn", "batch": B, "features": "logmel_iv", "channels": ds.n_channels, "graph_step": bool(graphed),
                "windows": len(ds), "rounds": rounds, "steps_per_round": steps,
                "ms_per_step_off": [round(v, 4) for v in off], "ms_per_step_on": [round(v, 4) for v in onn],
                "median_off_ms": round(med_off, 4), "median_on_ms": round(med_on, 4), "on_minus_off_ms": round(med_on - med_off, 4),
                "spread_ms": round(spread, 4), "difference_inside_spread": bool(abs(med_on - med_off) <= spread)}
    finally:
        Config.FEATURE_SET = saved


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None)
    ap.add_argument("--frames", type=int, default=120000, help="timeline length (40 min of audio)")
    ap.add_argument("--bursts", type=int, default=30)
    ap.add_argument("--burst-len", type=int, default=40, help="launches (and batch buffers) per burst: 40 x 8 MB at C = 4")
    ap.add_argument("--skip-e2e", action="store_true")
    ap.add_argument("--e2e-rounds", type=int, default=8)
    ap.add_argument("--e2e-steps", type=int, default=12)
    ap.add_argument("--profile", default=None, choices=CASES, help="short run of one case at C = 4, 7 and 36 for rocprofv3")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_spectral.py measures on the GPU: no ROCm device visible")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    if args.profile:
        doc = {"profile_case": args.profile,
               "kernels": [bench_kernels(dev, c, args.frames, 5, args.burst_len, only=args.profile) for c in (4, 7, 36)]}
    else:
        doc = {"shape": {"B": B, "window": WINDOW},
               "kernels": [bench_kernels(dev, c, args.frames, args.bursts, args.burst_len) for c in (4, 7, 36)]}
        doc["end_to_end"] = None if args.skip_e2e else bench_end_to_end(dev, args.e2e_rounds, args.e2e_steps)
    text = json.dumps(doc, indent=1)
    print(text)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
