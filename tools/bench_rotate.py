#!/usr/bin/env python
"""Cost of the rotation augmentation in azimuth steps (csrc/rotate.hip), on the GPU.

  python tools/bench_rotate.py                      kernels + end to end, one JSON document (also --out FILE)
  python tools/bench_rotate.py --skip-e2e           kernels only

Kernels, at the training shape (B = 32 windows of 250 frames, C_total = 4 and 7): the rotating pair (gather_rotate_kernel +
permute_mask_kernel<true>, the label kernel of csrc/augment.hip with the azimuth step) with the rows training draws under
AUGMENT_ROTATE against the augmenting pair of csrc/augment.hip (gather_augment_kernel + permute_mask_kernel<false>) with the
rows it draws under AUGMENT_SPATIAL -- both with two time and two frequency masks -- on the same starts, alternating in one
process.  Built the way tools/bench_augment.py is (its Burst is
used): a timed sample is a burst of launches captured as one HIP graph and replayed between two device events, every launch
with its own random starts; the timeline is larger than the Infinity Cache.  Bytes are the algorithm's: every output byte
written once and read once, and on the rotated path the three rotation-term rows read in place of the X and Y log-mel rows
(2304 B per frame at C = 4 against 2048 B; 35 of 36 drawn steps take that path).

End to end: full-size CRNN, batch 32, captured training steps fed by SELDDataset.device_batch on a dataset constructed with
the switch on, rotation off and on in alternating rounds of the same process; the on side includes the host draw and the
parameter upload.
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

from bench_augment import B, HBM_PEAK, I, J, WINDOW, Burst  # noqa: E402

MASKS = dict(AUGMENT_TIME_MASKS=2, AUGMENT_TIME_MASK_MAX=40, AUGMENT_FREQ_MASKS=2, AUGMENT_FREQ_MASK_MAX=12)


def bench_kernels(dev, channels, frames, bursts, burst_len):
    import seld_augment
    import seld_native as nat
    rng = np.random.default_rng(channels)
    spec_tm = torch.randn(frames, channels, 64, device=dev) * 30
    rot_tm = torch.rand(frames, 3, 64, device=dev) + 0.5             # P_X, P_Y > |C|: the combinations stay positive
    rot_tm[:, 2] -= 1.0
    mask_tm = torch.from_numpy(np.where(rng.random((frames, I * J)) < 0.03, 1 << rng.integers(0, 13, (frames, I * J)), 0)
                               .astype(np.uint16)).to(dev)
    feature_set = "logmel" if channels == 4 else "logmel_iv"
    table = seld_augment.channel_table(feature_set, channels)
    starts = [torch.from_numpy(rng.integers(0, frames - WINDOW, B)).to(dev) for _ in range(burst_len)]
    spec_out = torch.empty(B, WINDOW, channels, 64, device=dev)
    mask_out = torch.empty(B, WINDOW, I * J, dtype=torch.uint16, device=dev)
    seed = int(rng.integers(1 << 20))
    drawn = seld_augment.draw(seed, 1, np.arange(B), SimpleNamespace(AUGMENT_SPATIAL=True, **MASKS), window=WINDOW)
    turned = seld_augment.draw(seed, 1, np.arange(B), SimpleNamespace(AUGMENT_ROTATE=True, **MASKS), window=WINDOW, steps=J)
    rotated_windows = int((turned[:, 9] % (J // 4) != 0).sum())
    p_aug = nat.augment_params(drawn, B, WINDOW, dev)
    p_rot = nat.augment_params(turned, B, WINDOW, dev, steps=J)
    out_bytes = spec_out.numel() * 4
    per_frame_extra = 3 * 256 - 2 * 256                               # rotated path: three term rows read, two log-mel rows not
    rot_bytes = 2 * out_bytes + rotated_windows * WINDOW * per_frame_extra
    nbytes = {"augment_spec": 2 * out_bytes, "rotate_spec": rot_bytes, "augment_labels": 2 * mask_out.numel() * 2,
              "rotate_labels": 2 * mask_out.numel() * 2}
    fns = {
        "augment_spec": lambda s: nat.gather_windows_augment(spec_tm, s, WINDOW, p_aug, table, channels, 0.0, out=spec_out),
        "rotate_spec": lambda s: nat.gather_windows_rotate(spec_tm, rot_tm, s, WINDOW, p_rot, table, "WYZX", J, channels, 0.0,
                                                           out=spec_out),
        "augment_labels": lambda s: nat.gather_windows_permute(mask_tm, s, WINDOW, p_aug, I, J, out=mask_out),
        "rotate_labels": lambda s: nat.gather_windows_permute_rotate(mask_tm, s, WINDOW, p_rot, I, J, out=mask_out),
    }
    runs = {k: Burst(fn, starts) for k, fn in fns.items()}
    for run in runs.values():                                          # warm up every graph
        run.us_per_launch()
    samples = {k: [] for k in fns}
    for _ in range(bursts):                                            # alternate the four inside every round
        for k, run in runs.items():
            samples[k].append(run.us_per_launch())
    row = {}
    for k, v in samples.items():
        med = statistics.median(v)
        row[k] = {"us_per_launch_median": round(med, 3), "us_min": round(min(v), 3), "us_max": round(max(v), 3),
                  "bytes_moved": nbytes[k], "bytes_per_s": round(nbytes[k] / (med * 1e-6), 0),
                  "share_of_8TBps": round(nbytes[k] / (med * 1e-6) / HBM_PEAK, 4)}
    med = {k: row[k]["us_per_launch_median"] for k in row}
    row["ratio_spec"] = round(med["rotate_spec"] / med["augment_spec"], 3)
    row["ratio_labels"] = round(med["rotate_labels"] / med["augment_labels"], 3)
    row["ratio_pair"] = round((med["rotate_spec"] + med["rotate_labels"]) / (med["augment_spec"] + med["augment_labels"]), 3)
    row["byte_ratio_spec"] = round(rot_bytes / (2 * out_bytes), 3)
    return {"channels": channels, "timeline_frames": frames, "bursts": bursts, "launches_per_burst": burst_len,
            "rotated_windows_of_32": rotated_windows, "drawn": row}


def bench_end_to_end(dev, rounds, steps, features):
    """Captured CRNN bs-32 training steps on a dataset that holds rotation terms, AUGMENT_ROTATE off / on in alternating rounds."""
    import dataset
    import seld_augment
    import trainer
    from config import Config
    cfg = trainer.config
    saved = Config.FEATURE_SET, Config.AUGMENT_ROTATE
    Config.FEATURE_SET, Config.AUGMENT_ROTATE = features, True
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
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ds = dataset.SELDDataset.from_pcm(clips, rows, device=dev)
        torch.cuda.synchronize()
        construction_s = time.perf_counter() - t0
        Config.AUGMENT_ROTATE = False
        model = trainer.prepare_model_for_device(trainer.build_model((ds.I, ds.J), n_channels=ds.n_channels), dev).train()
        trainer.enable_master_weights(model, dev)
        graphed = trainer.graph_step_enabled(dev, 1)
        weights = torch.ones(14, device=dev)
        weights[13] = 0.05
        crit = trainer.SMRSELDLoss(loss_type="mse", w_class=1.0, grid_size=(ds.I, ds.J), class_weights=weights)
        opt = trainer.make_optimizer(model, cfg.LEARNING_RATE, dev, capturable=graphed)
        stepper = trainer.make_stepper(model, crit, opt, dev, 1)
        aug_cfg = SimpleNamespace(AUGMENT_ROTATE=True, **MASKS)
        order = np.random.default_rng(1).permutation(len(ds))

        def run(on, epoch):
            static = getattr(stepper, "static_inputs", None)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for n in range(steps):
                idx = order[(n * B) % (len(ds) - B):][:B]
                params = seld_augment.draw(3, epoch, idx, aug_cfg, window=WINDOW, steps=J) if on else None
                spec, mask = ds.device_batch(idx, out=static, augment=params)
                stepper(spec, mask)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3 / steps

        for on in (False, True, False, True):                           # capture + warm both paths
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
                "construction_with_terms_s": round(construction_s, 3),
                "rotation_terms_bytes": int(ds.rot_tm.numel() * 4), "feature_timeline_bytes": int(ds.spec_tm.numel() * 4),
                "ms_per_step_off": [round(v, 4) for v in off], "ms_per_step_on": [round(v, 4) for v in onn],
                "median_off_ms": round(med_off, 4), "median_on_ms": round(med_on, 4), "on_minus_off_ms": round(med_on - med_off, 4),
                "spread_ms": round(spread, 4), "difference_inside_spread": bool(abs(med_on - med_off) <= spread)}
    finally:
        Config.FEATURE_SET, Config.AUGMENT_ROTATE = saved


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
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_rotate.py measures on the GPU: no ROCm device visible")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
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
