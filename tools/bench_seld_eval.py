"""Cost of the SELD evaluation path (csrc/seld_eval.hip, seld_eval.py) against the model it evaluates.

Part 1, kernels: seeded bf16 logits of 32 clips x 60 s (1 920 windows, CRNN output shape [250, 648, 14]) decoded in
the streaming pattern of evaluate_seld (batches of 16 windows plus the 5 kept before them, views of one buffer), then
matched against synthetic references; the CRNN's eval-mode forward timed in the same process on batches of 16.
Gate: (decode + match) per window <= 10 % of the forward per window.  Run it under `rocprofv3 --kernel-trace --stats`
for the kernels' own durations (the HBM share of the decode: algorithmic bytes / kernel time / 8 TB/s).

Part 2, end to end: on one seeded CRNN checkpoint and one synthetic test set, trainer.test_model(save_visualizations=
False) and trainer.evaluate_seld alternate --repeats times; the medians are compared (gate: <= 1.10).

    python tools/bench_seld_eval.py --out profiles/seld_eval.json
"""
import argparse
import json
import statistics
import sys
import tempfile
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "sound-event-localization-detection_amd"))

import seld_eval  # noqa: E402
import trainer  # noqa: E402

WINDOW_BYTES_BF16 = 250 * 648 * 14 * 2


def synthetic_rows(rng, n_frames, per_meta=2):
    n_meta = (n_frames + 4) // 5
    rows = []
    for m in range(n_meta):
        for s in range(int(rng.integers(0, 2 * per_meta + 1))):
            rows.append([m, int(rng.integers(0, 13)), s, int(rng.integers(-180, 180)), int(rng.integers(-90, 91))])
    return np.array(rows, dtype=np.int64).reshape(-1, 5)


def crnn(device):
    trainer.config.MODEL_TYPE = "crnn"
    torch.manual_seed(0)
    return trainer.prepare_model_for_device(trainer.build_model((18, 36), True, n_channels=4), device).eval()


def time_events(fn, iters):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) * 1e3 / iters          # microseconds per call of fn


def kernels(args, device):
    frames = args.seconds * 50
    segments = np.stack([np.arange(args.clips) * frames, np.full(args.clips, frames)], 1)
    table = seld_eval.meta_frame_table(segments)
    n_w = table.windows
    gen = torch.Generator(device=device).manual_seed(1234)
    logits = torch.empty((n_w, 250, 648, 14), dtype=torch.bfloat16, device=device)
    for lo in range(0, n_w, 64):
        logits[lo:lo + 64] = torch.randn((min(64, n_w - lo), 250, 648, 14), generator=gen, device=device,
                                         dtype=torch.float32).to(torch.bfloat16)
    logits[..., 13] += 4.0
    k = 4
    det = (torch.empty((len(table), 13, k), dtype=torch.int32, device=device),
           torch.empty((len(table), 13, k), dtype=torch.float32, device=device),
           torch.empty((len(table), 13), dtype=torch.int32, device=device))
    b = args.batch
    plan = []                                   # (w0, w1, q0, q1) of each streaming step
    done = 0
    for lo in range(0, n_w, b):
        hi = min(lo + b, n_w)
        end = int(np.searchsorted(table.last_window, hi - 1, side="right"))
        plan.append((max(0, lo - seld_eval.KEEP_WINDOWS), hi, done, end))
        done = end

    def decode_all():
        for w0, w1, q0, q1 in plan:
            if q1 > q0:
                seld_eval.grid_decode(logits[w0:w1], w0, table, q0, q1 - q0, 0.5, k,
                                      out=(det[0][q0:q1], det[1][q0:q1], det[2][q0:q1]))

    rng = np.random.default_rng(7)
    rows = [synthetic_rows(rng, frames) for _ in range(args.clips)]
    offsets, dirs = seld_eval.reference_table(table, rows)
    offsets_d, dirs_d = torch.from_numpy(offsets).to(device), torch.from_numpy(dirs).to(device)

    def match_all():
        seld_eval.doa_match(det[0], det[2], offsets_d, dirs_d, 20.0)

    decode_all()
    match_all()
    decode_us = time_events(decode_all, args.iters) / n_w
    match_us = time_events(match_all, args.iters) / n_w
    detections = int(det[2].sum())
    del logits

    model = crnn(device)
    spec = torch.randn((b, 250, 4, 64), generator=gen, device=device)

    def forward():
        with torch.no_grad(), trainer.autocast_context(device):
            model(spec)

    for _ in range(3):
        forward()
    forward_us = time_events(forward, args.iters) / b
    ratio = (decode_us + match_us) / forward_us
    return {"windows": n_w, "meta_frames": len(table), "batch": b, "max_peaks": k, "detections": detections,
            "references": int(offsets[-1]), "decode_us_per_window": decode_us, "match_us_per_window": match_us,
            "crnn_eval_forward_us_per_window": forward_us, "eval_over_forward": ratio, "gate_eval_over_forward": 0.10,
            "decode_algorithmic_bytes": n_w * WINDOW_BYTES_BF16 + len(table) * 13 * (2 * k + 1) * 4,
            "decode_hbm_share_event_timed": (n_w * WINDOW_BYTES_BF16) / (decode_us * n_w * 1e-6) / 8e12}


def end_to_end(args, device):
    from torch.utils.data import DataLoader
    import dataset
    from oracle import features as ofeat
    n = 24000 * args.seconds
    clips = [ofeat.synth_pcm(i, 4, n, "noise") for i in range(args.e2e_clips)]
    rng = np.random.default_rng(3)
    rows = [synthetic_rows(rng, n // 480) for _ in clips]
    ds = dataset.SELDDataset.from_pcm(clips, rows, device=device, use_gaussian_augmentation=False)
    loader = DataLoader(ds, batch_size=args.batch, shuffle=False)
    model = crnn(device)
    tmp = Path(tempfile.mkdtemp())
    path = tmp / "crnn.pth"
    torch.save({"epoch": 0, "model_state_dict": trainer.model_state_dict(model), "train_loss": 0.0, "test_loss": 0.0,
                "config": trainer.config}, path)
    times = {"test_model": [], "evaluate_seld": []}
    result = None
    for _ in range(args.repeats):
        for name in ("test_model", "evaluate_seld"):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if name == "test_model":
                trainer.test_model(loader, model_path=path, device=device, save_visualizations=False)
            else:
                result = trainer.evaluate_seld(loader, model_path=path, device=device, threshold=1.0 / 14.0 + 1e-4)
            torch.cuda.synchronize()
            times[name].append(time.perf_counter() - t0)
    med = {k: statistics.median(v) for k, v in times.items()}
    return {"windows": len(ds), "clips": args.e2e_clips, "seconds_per_clip": args.seconds, "batch": args.batch,
            "times_s": times, "median_s": med, "evaluate_over_test_model": med["evaluate_seld"] / med["test_model"],
            "gate_evaluate_over_test_model": 1.10,
            "metrics_untrained": {k: result[k] for k in ("F20", "ER20", "LE_CD", "LR_CD", "TP", "FP", "FN", "N")}}


def main():
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--clips", type=int, default=32)
    p.add_argument("--seconds", type=int, default=60)
    p.add_argument("--batch", type=int, default=16)
    p.add_argument("--iters", type=int, default=5)
    p.add_argument("--e2e-clips", type=int, default=8)
    p.add_argument("--repeats", type=int, default=3)
    p.add_argument("--skip-e2e", action="store_true")
    p.add_argument("--out", default=None)
    args = p.parse_args()
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    out = {"device": torch.cuda.get_device_name(0), "kernels": kernels(args, device)}
    print(json.dumps(out["kernels"]), flush=True)
    if not args.skip_e2e:
        out["end_to_end"] = end_to_end(args, device)
        print(json.dumps(out["end_to_end"]), flush=True)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(out, indent=2) + "\n")


if __name__ == "__main__":
    main()
