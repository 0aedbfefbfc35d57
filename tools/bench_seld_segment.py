"""Cost of the segment-based SELD metrics (csrc/seld_segment.hip, seld_eval.segment_metrics).

On the seeded timeline of DESIGN.md 10.4 (bf16 logits of 32 clips x 60 s, 1 920 windows, decoded in the streaming pattern
of evaluate_seld at K = 4, synthetic references) the three new launches are timed next to the decode, the matcher and the
CRNN's eval-mode forward in one process, HIP events, medians over --repeats rounds that alternate the forms:
  decode, match                       as tools/bench_seld_eval.py times them
  assign, segment_score, jackknife    seld_doa_assign, seld_segment_score (both launches), seld_jackknife_score
  segment_metrics                     the host function around the three (reference upload excluded, host copies included)
Gate (with the new kernels in the numerator): (decode + match + assign + segment_score + jackknife) per
window <= 10 % of the forward per window.  Random logits leave few detections, so the three kernels are also timed on
"dense" detections of the same timeline: 0..4 per (meta-frame, class) at random cells, references near them.

    python tools/bench_seld_segment.py --out profiles/seld_segment.json
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "sound-event-localization-detection_amd"))
sys.path.insert(0, str(ROOT / "tools"))

import seld_eval  # noqa: E402
import trainer  # noqa: E402
from bench_seld_eval import crnn, synthetic_rows  # noqa: E402


def timed(fn):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) * 1e3                   # microseconds


def dense_detections(table, k, device):
    """(det_cell int32 [Q, 13, K], det_count int32 [Q, 13], reference rows per clip): 0..K detections per (q, c) on distinct
    cells, and for seven in ten of them a reference within a few degrees (one in four of those up to 30 degrees off)."""
    rng = np.random.default_rng(11)
    q_n = len(table)
    count = rng.integers(0, k + 1, size=(q_n, 13)).astype(np.int32)
    start, step = rng.integers(0, 648, size=(q_n, 13, 1)), rng.integers(1, 648 // k, size=(q_n, 13, 1))
    cell = ((start + step * np.arange(k)) % 648).astype(np.int32)                  # (k step < 648: distinct cells)
    cell[np.arange(k) >= count[..., None]] = -1
    rows = [[] for _ in range(len(table.seg_offsets) - 1)]
    q_idx, c_idx, r_idx = np.nonzero((np.arange(k) < count[..., None]) & (rng.random((q_n, 13, k)) < 0.7))
    spread = np.where(rng.random(len(q_idx)) < 0.25, 30, 4)
    x = cell[q_idx, c_idx, r_idx].astype(np.int64)
    az = np.clip(-175 + 10 * (x % 36) + rng.integers(-spread, spread + 1), -180, 180)
    el = np.clip(-85 + 10 * (x // 36) + rng.integers(-spread, spread + 1), -90, 90)
    for q, c, r, a, e in zip(q_idx, c_idx, r_idx, az, el):
        rows[int(table.segment[q])].append([int(table.index[q]), int(c), int(r), int(a), int(e)])
    rows = [np.array(r, dtype=np.int64).reshape(-1, 5) for r in rows]
    return torch.from_numpy(cell).to(device), torch.from_numpy(count).to(device), rows


def run(args, device):
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
    k, b = 4, args.batch
    det = (torch.empty((len(table), 13, k), dtype=torch.int32, device=device),
           torch.empty((len(table), 13, k), dtype=torch.float32, device=device),
           torch.empty((len(table), 13), dtype=torch.int32, device=device))
    plan, done = [], 0                          # (w0, w1, q0, q1) of each streaming step
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
    refs = seld_eval.device_references(table, rows, device)
    decode_all()
    dense_cell, dense_count, dense_rows = dense_detections(table, k, device)
    dense_refs = seld_eval.device_references(table, dense_rows, device)
    model = crnn(device)
    spec = torch.randn((b, 250, 4, 64), generator=gen, device=device)

    def forward():
        with torch.no_grad(), trainer.autocast_context(device):
            model(spec)

    def forms_for(cell, count, rf, rws):
        pair = seld_eval.doa_assign(cell, count, rf[0], rf[1], 20.0)
        scored = seld_eval.segment_score(pair, count, k, rf[0], table, 20.0)
        return {"match": lambda: seld_eval.doa_match(cell, count, rf[0], rf[1], 20.0),
                "assign": lambda: seld_eval.doa_assign(cell, count, rf[0], rf[1], 20.0),
                "segment_score": lambda: seld_eval.segment_score(pair, count, k, rf[0], table, 20.0),
                "jackknife": lambda: seld_eval.jackknife_score(*scored[2:]),
                "segment_metrics": lambda: seld_eval.segment_metrics(cell, count, table, rws, 20.0, refs=rf, jackknife=True)}

    forms = {"decode": decode_all, "forward": forward}
    forms.update(forms_for(det[0], det[2], refs, rows))
    forms.update({f"dense_{name}": fn for name, fn in forms_for(dense_cell, dense_count, dense_refs, dense_rows).items()})
    for fn in forms.values():                   # warm-up
        fn()
    times = {name: [] for name in forms}
    for _ in range(args.repeats):
        for name, fn in forms.items():
            times[name].append(timed(fn))
    med = {name: statistics.median(v) for name, v in times.items()}
    forward_us = med["forward"] / b
    new = med["assign"] + med["segment_score"] + med["jackknife"]
    dense_new = med["dense_assign"] + med["dense_segment_score"] + med["dense_jackknife"]
    sparse = seld_eval.segment_metrics(det[0], det[2], table, rows, 20.0, refs=refs, jackknife=True)
    dense = seld_eval.segment_metrics(dense_cell, dense_count, table, dense_rows, 20.0, refs=dense_refs, jackknife=True)
    return {"windows": n_w, "meta_frames": len(table), "recordings": args.clips, "blocks": sparse["blocks"], "batch": b,
            "max_peaks": k, "repeats": args.repeats, "detections": int(det[2].sum()), "references": int(refs[0][-1]),
            "dense_detections": int(dense_count.sum()), "dense_references": int(dense_refs[0][-1]),
            "median_us": med, "times_us": times,
            "decode_us_per_window": med["decode"] / n_w, "match_us_per_window": med["match"] / n_w,
            "segment_kernels_us_per_window": new / n_w, "dense_segment_kernels_us_per_window": dense_new / n_w,
            "crnn_eval_forward_us_per_window": forward_us,
            "eval_over_forward": (med["decode"] + med["match"] + new) / n_w / forward_us,
            "dense_eval_over_forward": (med["decode"] + med["dense_match"] + dense_new) / n_w / forward_us,
            "gate_eval_over_forward": 0.10,
            "macro": sparse["macro"], "dense_macro": dense["macro"], "dense_counts": dense["counts"],
            "dense_ci_macro_SELD": dense["ci"]["macro"]["SELD"]}


def main():
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--clips", type=int, default=32)
    p.add_argument("--seconds", type=int, default=60)
    p.add_argument("--batch", type=int, default=16)
    p.add_argument("--repeats", type=int, default=7)
    p.add_argument("--out", default=None)
    args = p.parse_args()
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    out = {"device": torch.cuda.get_device_name(0), "kernels": run(args, device)}
    print(json.dumps({k: v for k, v in out["kernels"].items() if k != "times_us"}), flush=True)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(out, indent=2) + "\n")


if __name__ == "__main__":
    main()
