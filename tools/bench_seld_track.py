"""Cost of track linking in the SELD evaluation (csrc/seld_track.hip).

The workload of tools/bench_seld_eval.py -- seeded bf16 logits of 32 clips x 60 s, 1 920 windows, 19 200 meta-frames,
decoded in the streaming pattern of evaluate_seld -- with sources planted into the logits so that the decode has
something to hand on: per (clip, class) chain two sources that drift by single cells and drop out now and then, plus
clutter.  416 chains of 600 meta-frames.

  kernels   decode (all streaming calls), track (seld_eval.track: the prefix sums, the one host read, both launches) and
            match, each per timeline between device events, the candidates taking turns; the CRNN's eval forward on
            batches of 16 windows in the same rounds.  Gate (10.4): (decode + track + match) <= 10 % of the forward.
  e2e       trainer.evaluate_seld with tracking off and on, alternating, on a synthetic test set.

Every step runs in a child process of its own under a time limit; a failed step ends the run.  One JSON line per step on
stdout, all of them in --out.

    python tools/bench_seld_track.py --out profiles/r11_seld_track.json
    rocprofv3 --kernel-trace --stats -- python tools/bench_seld_track.py --step kernels        (kernel durations proper)
"""
import argparse
import json
import statistics
import subprocess
import sys
import tempfile
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "sound-event-localization-detection_amd"))

STEP_LIMIT_S = {"kernels": 420, "e2e": 420}


def planted_sources(rng, clips, n_meta, sources=2, dropout=0.1, clutter=0.05):
    """(segment, m, class, cell) int64 arrays of the planted detections: per (clip, class) ``sources`` random walks over
    the 18 x 36 grid (one cell per meta-frame in each direction at most, azimuth wraps), each missing from a frame with
    probability ``dropout``, and one clutter cell with probability ``clutter``."""
    import numpy as np
    chains = clips * 13
    start_i = rng.integers(0, 18, size=(chains, sources, 1))
    start_j = rng.integers(0, 36, size=(chains, sources, 1))
    i = np.clip(start_i + np.cumsum(rng.integers(-1, 2, size=(chains, sources, n_meta)), -1), 0, 17)
    j = (start_j + np.cumsum(rng.integers(-1, 2, size=(chains, sources, n_meta)), -1)) % 36
    keep = rng.uniform(size=i.shape) >= dropout
    x, _, m = np.nonzero(keep)
    cell = (i * 36 + j)[keep]
    cx, cm = np.nonzero(rng.uniform(size=(chains, n_meta)) < clutter)
    x, m = np.concatenate([x, cx]), np.concatenate([m, cm])
    cell = np.concatenate([cell, rng.integers(0, 648, size=len(cx))])
    return x // 13, m, x % 13, cell


def time_events(fn, iters):
    import torch
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) * 1e3 / iters          # microseconds per call of fn


def summary(samples):
    return {"median_us": statistics.median(samples), "min_us": min(samples), "max_us": max(samples), "samples_us": samples}


def crnn(device):
    import torch
    import trainer
    trainer.config.MODEL_TYPE = "crnn"
    torch.manual_seed(0)
    return trainer.prepare_model_for_device(trainer.build_model((18, 36), True, n_channels=4), device).eval()


def synthetic_rows(rng, n_frames, per_meta=2):
    import numpy as np
    n_meta = (n_frames + 4) // 5
    rows = []
    for m in range(n_meta):
        for s in range(int(rng.integers(0, 2 * per_meta + 1))):
            rows.append([m, int(rng.integers(0, 13)), s, int(rng.integers(-180, 180)), int(rng.integers(-90, 91))])
    return np.array(rows, dtype=np.int64).reshape(-1, 5)


def kernels(args):
    import numpy as np
    import torch
    import seld_eval
    import trainer
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    frames = args.seconds * 50
    n_meta = frames // 5
    segments = np.stack([np.arange(args.clips) * frames, np.full(args.clips, frames)], 1)
    table = seld_eval.meta_frame_table(segments)
    n_w = table.windows
    gen = torch.Generator(device=device).manual_seed(1234)
    logits = torch.empty((n_w, 250, 648, 14), dtype=torch.bfloat16, device=device)
    for lo in range(0, n_w, 64):
        logits[lo:lo + 64] = torch.randn((min(64, n_w - lo), 250, 648, 14), generator=gen, device=device,
                                         dtype=torch.float32).to(torch.bfloat16)
    logits[..., 13] += 4.0
    seg, m, cls, cell = planted_sources(np.random.default_rng(11), args.clips, n_meta)
    f = (seg * frames + 5 * m)[:, None] + np.arange(5)[None, :]                    # the 5 frames of each meta-frame
    w = f[..., None] // 50 - np.arange(5)[None, None, :]                           # the windows that cover them
    ok = (w >= 0) & (w < n_w)
    row = f[..., None] - 50 * w
    pick = lambda a: torch.from_numpy(np.broadcast_to(a, w.shape)[ok]).to(device)
    logits[pick(w), pick(row), pick(cell[:, None, None]), pick(cls[:, None, None])] = 12.0
    k = args.max_peaks
    det = (torch.empty((len(table), 13, k), dtype=torch.int32, device=device),
           torch.empty((len(table), 13, k), dtype=torch.float32, device=device),
           torch.empty((len(table), 13), dtype=torch.int32, device=device))
    b = args.batch
    plan, done = [], 0                         # (w0, w1, q0, q1) of each streaming step
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

    settings = {"gate_deg": args.gate_deg, "max_gap": args.max_gap, "min_len": args.min_len}
    linked = {}

    def track_all():
        linked["out"] = seld_eval.track(det[0], det[2], table, settings["gate_deg"], settings["max_gap"],
                                        settings["min_len"])

    rng = np.random.default_rng(7)
    offsets, dirs = seld_eval.reference_table(table, [synthetic_rows(rng, frames) for _ in range(args.clips)])
    offsets_d, dirs_d = torch.from_numpy(offsets).to(device), torch.from_numpy(dirs).to(device)

    def match_all():
        seld_eval.doa_match(linked["out"][0], linked["out"][2], offsets_d, dirs_d, 20.0)

    model = crnn(device)
    spec = torch.randn((b, 250, 4, 64), generator=gen, device=device)

    def forward_all():                         # the forwards of the same windows: n_w / b batches
        with torch.no_grad(), trainer.autocast_context(device):
            for _ in range((n_w + b - 1) // b):
                model(spec)

    decode_all()
    track_all()
    match_all()
    forward_all()
    fns = {"decode": decode_all, "track": track_all, "match": match_all, "crnn_eval_forward": forward_all}
    samples = {name: [] for name in fns}
    for _ in range(args.repeats):
        for name, fn in fns.items():
            samples[name].append(time_events(fn, args.iters))
    out = {name: summary(v) for name, v in samples.items()}
    med = {name: out[name]["median_us"] for name in fns}
    counts = seld_eval.track_summary(linked["out"][2], linked["out"][3], linked["out"][4])
    out.update({"device": torch.cuda.get_device_name(0), "windows": n_w, "meta_frames": len(table), "chains": args.clips * 13,
                "frames_per_chain": n_meta, "batch": b, "max_peaks": k, "iters": args.iters, "repeats": args.repeats,
                "settings": settings, "detections": int(det[2].sum()), "planted": int(len(cell)), **counts,
                "emissions": int(linked["out"][2].sum()), "references": int(offsets[-1]),
                "track_us_per_timeline": med["track"],
                "track_over_decode_plus_match": med["track"] / (med["decode"] + med["match"]),
                "track_over_forward": med["track"] / med["crnn_eval_forward"],
                "decode_track_match_over_forward": (med["decode"] + med["track"] + med["match"]) / med["crnn_eval_forward"],
                "decode_match_over_forward": (med["decode"] + med["match"]) / med["crnn_eval_forward"],
                "gate_eval_over_forward": 0.10})
    return out


def end_to_end(args):
    import numpy as np
    import torch
    from torch.utils.data import DataLoader
    import dataset
    import trainer
    from oracle import features as ofeat
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    n = 24000 * args.seconds
    clips = [ofeat.synth_pcm(i, 4, n, "noise") for i in range(args.e2e_clips)]
    rng = np.random.default_rng(3)
    rows = [synthetic_rows(rng, n // 480) for _ in clips]
    ds = dataset.SELDDataset.from_pcm(clips, rows, device=device, use_gaussian_augmentation=False)
    loader = DataLoader(ds, batch_size=args.batch, shuffle=False)
    model = crnn(device)
    path = Path(tempfile.mkdtemp()) / "crnn.pth"
    torch.save({"epoch": 0, "model_state_dict": trainer.model_state_dict(model), "train_loss": 0.0, "test_loss": 0.0,
                "config": trainer.config}, path)
    track = {"gate_deg": args.gate_deg, "max_gap": args.max_gap, "min_len": args.min_len}
    run = lambda tr: trainer.evaluate_seld(loader, model_path=path, device=device, threshold=1.0 / 14.0 + 1e-4,
                                           max_peaks=args.max_peaks, track=tr)
    run(False)                                 # first-use costs
    times, results = {"off": [], "on": []}, {}
    for _ in range(args.repeats):
        for name, tr in (("off", False), ("on", track)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            results[name] = run(tr)
            torch.cuda.synchronize()
            times[name].append(time.perf_counter() - t0)
    med = {k: statistics.median(v) for k, v in times.items()}
    keys = ("F20", "ER20", "LE_CD", "LR_CD", "TP", "FP", "FN", "N")
    return {"windows": len(ds), "clips": args.e2e_clips, "seconds_per_clip": args.seconds, "batch": args.batch,
            "times_s": times, "median_s": med, "on_over_off": med["on"] / med["off"], "tracking": results["on"]["tracking"],
            "metrics_untrained": {name: {k: results[name][k] for k in keys} for name in results}}


def main():
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--clips", type=int, default=32)
    p.add_argument("--seconds", type=int, default=60)
    p.add_argument("--batch", type=int, default=16)
    p.add_argument("--max-peaks", type=int, default=4)
    p.add_argument("--gate-deg", type=float, default=20.0)
    p.add_argument("--max-gap", type=int, default=2)
    p.add_argument("--min-len", type=int, default=3)
    p.add_argument("--iters", type=int, default=5)
    p.add_argument("--repeats", type=int, default=5)
    p.add_argument("--e2e-clips", type=int, default=8)
    p.add_argument("--step", choices=sorted(STEP_LIMIT_S), default=None,
                   help="run this step here, in this process (what the driver starts; also the form to profile)")
    p.add_argument("--skip-e2e", action="store_true")
    p.add_argument("--out", default=None)
    args = p.parse_args()
    if args.step:
        print(json.dumps({args.step: kernels(args) if args.step == "kernels" else end_to_end(args)}), flush=True)
        return 0
    out = {"command": "python tools/bench_seld_track.py " + " ".join(sys.argv[1:])}
    forwarded = [a for a in sys.argv[1:]]
    for flag in ("--out", "--step"):
        if flag in forwarded:
            at = forwarded.index(flag)
            del forwarded[at:at + 2]
    forwarded = [a for a in forwarded if a != "--skip-e2e"]
    for step in ("kernels",) + (() if args.skip_e2e else ("e2e",)):
        try:
            run = subprocess.run([sys.executable, str(Path(__file__).resolve()), "--step", step, *forwarded],
                                 capture_output=True, text=True, timeout=STEP_LIMIT_S[step])
        except subprocess.TimeoutExpired:
            print(f"step {step} exceeded {STEP_LIMIT_S[step]} s; stopping", file=sys.stderr)
            return 124
        if run.returncode != 0:
            print(run.stdout[-2000:], run.stderr[-4000:], file=sys.stderr)
            print(f"step {step} failed with code {run.returncode}; stopping", file=sys.stderr)
            return run.returncode
        line = [ln for ln in run.stdout.splitlines() if ln.startswith("{")][-1]
        out.update(json.loads(line))
        print(line, flush=True)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(out, indent=2) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
