"""Cost of test-time augmentation in the SELD evaluation (csrc/seld_tta.hip).

One steady-state call of the streaming decode -- 16 new windows plus the 5 kept before them, 160 meta-frames -- on seeded
bf16 logits, for n = 1, 4 and 16 pattern stacks:

  (a) seld_grid_decode_tta at patterns = (0,) against seld_grid_decode on the same logits, alternating in one process;
      the run-to-run spread of the alternating samples is reported next to the difference
  (b) seld_grid_decode_tta against the framework-op form it replaces: softmax in fp32 -> index_select on the cell axis ->
      mean over the stacks -> log -> seld_grid_decode
  (c) decode + match as a share of the n eval forwards of the CRNN (batches of 16) they accompany; gate 10 % (10.4)
  (d) trainer.evaluate_seld(tta="all") against trainer.evaluate_seld() wall time, alternating, on a synthetic test set

    python tools/bench_seld_tta.py --out profiles/seld_tta.json
    rocprofv3 --kernel-trace --stats -- python tools/bench_seld_tta.py --n 1 --skip-e2e        (kernel durations proper)
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

import seld_augment  # noqa: E402
import seld_eval  # noqa: E402
import trainer  # noqa: E402

PATTERN_LISTS = {1: (0,), 4: (0, 3, 10, 13), 16: tuple(range(16))}


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


def alternate(fns, iters, repeats):
    """{name: [us per call, one sample per repeat]} with the candidates taking turns inside every repeat."""
    for fn in fns.values():
        fn()
    samples = {name: [] for name in fns}
    for _ in range(repeats):
        for name, fn in fns.items():
            samples[name].append(time_events(fn, iters))
    return samples


def summary(samples):
    return {"median_us": statistics.median(samples), "min_us": min(samples), "max_us": max(samples), "samples_us": samples}


def kernels(args, device):
    b, keep = args.batch, seld_eval.KEEP_WINDOWS
    n_w = 4 * b                                                   # a timeline long enough for one steady-state call
    table = seld_eval.meta_frame_table(np.array([[0, 50 * n_w]]))
    w0, w1 = 2 * b - keep, 3 * b                                  # the call that receives windows [2 b, 3 b)
    q0 = int(np.searchsorted(table.last_window, 2 * b - 1, side="right"))
    q1 = int(np.searchsorted(table.last_window, 3 * b - 1, side="right"))
    nq = q1 - q0
    k = 4
    gen = torch.Generator(device=device).manual_seed(1234)
    n_max = max(PATTERN_LISTS)
    logits = torch.empty((n_max, w1 - w0, 250, 648, 14), dtype=torch.bfloat16, device=device)
    for n in range(n_max):
        x = torch.randn((w1 - w0, 250, 648, 14), generator=gen, device=device, dtype=torch.float32)
        x[..., 13] += 4.0
        logits[n] = x.to(torch.bfloat16)
    del x

    def outputs():
        return (torch.empty((nq, 13, k), dtype=torch.int32, device=device),
                torch.empty((nq, 13, k), dtype=torch.float32, device=device),
                torch.empty((nq, 13), dtype=torch.int32, device=device))

    det, det_ops = outputs(), outputs()
    rng = np.random.default_rng(7)
    offsets, dirs = seld_eval.reference_table(table, [synthetic_rows(rng, 50 * n_w)])
    lo, hi = offsets[q0 * 13], offsets[q1 * 13]
    offsets_d = torch.from_numpy((offsets[q0 * 13:q1 * 13 + 1] - lo).astype(np.int32)).to(device)
    dirs_d = torch.from_numpy(dirs[lo:hi]).to(device)

    model = crnn(device)
    spec = torch.randn((b, 250, 4, 64), generator=gen, device=device)

    def forward():
        with torch.no_grad(), trainer.autocast_context(device):
            model(spec)

    for _ in range(3):
        forward()

    def match():
        seld_eval.doa_match(det[0], det[2], offsets_d, dirs_d, 20.0)

    out = {"batch": b, "kept_windows": keep, "windows_per_call": w1 - w0, "meta_frames_per_call": nq, "max_peaks": k,
           "iters": args.iters, "repeats": args.repeats, "per_n": {}}
    for n, patterns in PATTERN_LISTS.items():
        if args.n and n not in args.n:
            continue
        stacks = logits[:n]
        dest = [torch.from_numpy(seld_augment.cell_dest(p)).to(device) for p in patterns]

        def tta():
            seld_eval.grid_decode_tta(stacks, patterns, w0, table, q0, nq, 0.5, k, out=det)

        def framework_ops():
            acc = torch.softmax(stacks[0].float(), -1).index_select(2, dest[0])
            for i in range(1, n):
                acc += torch.softmax(stacks[i].float(), -1).index_select(2, dest[i])
            seld_eval.grid_decode(torch.log(acc / n), w0, table, q0, nq, 0.5, k, out=det_ops)

        fns = {"tta_kernel": tta, "framework_ops": framework_ops, "match": match, "crnn_eval_forward": forward}
        if n == 1:
            fns["plain_kernel"] = lambda: seld_eval.grid_decode(stacks[0], w0, table, q0, nq, 0.5, k, out=det_ops)
        samples = alternate(fns, args.iters, args.repeats)
        row = {name: summary(v) for name, v in samples.items()}
        row["patterns"] = list(patterns)
        row["logit_bytes_per_call"] = n * (w1 - w0) * 250 * 648 * 14 * 2
        row["tta_hbm_share_event_timed"] = row["logit_bytes_per_call"] / (row["tta_kernel"]["median_us"] * 1e-6) / 8e12
        row["framework_ops_over_tta_kernel"] = row["framework_ops"]["median_us"] / row["tta_kernel"]["median_us"]
        row["decode_and_match_over_n_forwards"] = (row["tta_kernel"]["median_us"] + row["match"]["median_us"]) / \
            (n * row["crnn_eval_forward"]["median_us"])
        row["gate_decode_and_match_over_n_forwards"] = 0.10
        if n == 1:
            t, p = samples["tta_kernel"], samples["plain_kernel"]
            row["tta_minus_plain_median_us"] = statistics.median(t) - statistics.median(p)
            row["spread_us"] = {"tta_kernel": max(t) - min(t), "plain_kernel": max(p) - min(p)}
            tta()
            row["bit_identical_to_plain"] = all(torch.equal(a, c) for a, c in zip(det, det_ops))
        out["per_n"][str(n)] = row
        print(json.dumps({"n": n, **{key: row[key] for key in row if not isinstance(row[key], dict)},
                          **{key: row[key]["median_us"] for key in fns}}), flush=True)
    return out


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
    path = Path(tempfile.mkdtemp()) / "crnn.pth"
    torch.save({"epoch": 0, "model_state_dict": trainer.model_state_dict(model), "train_loss": 0.0, "test_loss": 0.0,
                "config": trainer.config}, path)
    times = {"plain": [], "tta_all": []}
    results = {}
    for _ in range(args.repeats):
        for name, tta in (("plain", ()), ("tta_all", "all")):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            results[name] = trainer.evaluate_seld(loader, model_path=path, device=device, threshold=1.0 / 14.0 + 1e-4, tta=tta)
            torch.cuda.synchronize()
            times[name].append(time.perf_counter() - t0)
    med = {k: statistics.median(v) for k, v in times.items()}
    keys = ("F20", "ER20", "LE_CD", "LR_CD", "TP", "FP", "FN", "N")
    return {"windows": len(ds), "clips": args.e2e_clips, "seconds_per_clip": args.seconds, "batch": args.batch,
            "times_s": times, "median_s": med, "tta_all_over_plain": med["tta_all"] / med["plain"],
            "metrics_untrained": {name: {k: results[name][k] for k in keys} for name in results}}


def main():
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--batch", type=int, default=16)
    p.add_argument("--iters", type=int, default=20)
    p.add_argument("--repeats", type=int, default=7)
    p.add_argument("--seconds", type=int, default=60)
    p.add_argument("--e2e-clips", type=int, default=8)
    p.add_argument("--n", type=int, nargs="*", default=None, choices=sorted(PATTERN_LISTS),
                   help="pattern counts to time (default: all); one at a time under rocprofv3 --kernel-trace --stats")
    p.add_argument("--skip-e2e", action="store_true")
    p.add_argument("--out", default=None)
    args = p.parse_args()
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    out = {"device": torch.cuda.get_device_name(0), "kernels": kernels(args, device)}
    if not args.skip_e2e:
        out["end_to_end"] = end_to_end(args, device)
        print(json.dumps(out["end_to_end"]), flush=True)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(out, indent=2) + "\n")


if __name__ == "__main__":
    main()
