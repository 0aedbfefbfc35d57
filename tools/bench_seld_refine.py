"""Cost of the sub-cell DOA refinement in the SELD decode (csrc/seld_refine.hip).

The workload of tools/bench_seld_eval.py: seeded bf16 logits of 32 clips x 60 s (1 920 windows) decoded in the streaming
pattern of evaluate_seld -- 16 new windows per call plus the 5 kept before them, 160 meta-frames -- then matched against
synthetic references.  Those random logits decode to no detection at all, which would leave the refinement nothing to do,
so two sources per meta-frame are planted into them (+8 at a random cell and class, +6 at its azimuth neighbour: a peak
with a sub-cell offset), the same for every candidate.  Timed are the kernels' own durations from `rocprofv3 --kernel-trace --stats`, each sample a run of
its own:

  plain     seld_grid_decode          against   refined   seld_grid_decode_refine (plain walk), same logits
  match     seld_doa_match            against   dirs      seld_doa_match_dirs on the refined directions

and the yardstick: the plain grid_decode_kernel<bf16> of the PARENT commit, from a checkout of it built next to this one
(--parent-package: its sound-event-localization-detection_amd directory with libseld_hip.so in it).  Samples alternate
parent, this tree, parent, ...; inside a process the candidates take turns pass by pass.  Reported: the medians over the
samples of the per-process median launch, and the parent's own sample spread (max - min).

    python tools/bench_seld_refine.py --parent-package ../parent/sound-event-localization-detection_amd \\
        --out profiles/seld_refine.json
"""
import argparse
import csv
import json
import statistics
import subprocess
import sys
import tempfile
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
PACKAGE = ROOT / "sound-event-localization-detection_amd"
# substring of the traced kernel name -> candidate; the first that matches wins
KERNELS = (("refine_decode_kernel", "refined_decode"), ("grid_decode_kernel", "plain_decode"),
           ("doa_match_dirs_kernel", "match_dirs"), ("doa_match_kernel", "match"))


def synthetic_rows(rng, n_frames, per_meta=2):
    n_meta = (n_frames + 4) // 5
    rows = []
    for m in range(n_meta):
        for s in range(int(rng.integers(0, 2 * per_meta + 1))):
            rows.append([m, int(rng.integers(0, 13)), s, int(rng.integers(-180, 180)), int(rng.integers(-90, 91))])
    return rows


def plant_sources(logits, table, rng, device, per_meta=2):
    """Two sources per meta-frame into window logits [W, 250, 648, 14], in every window that covers its frames: +8 at a
    random (cell, class), +6 at the cell's neighbour in azimuth.  Returns the number of sources."""
    import numpy as np
    import torch
    n_w = int(logits.shape[0])
    q = np.repeat(np.arange(len(table)), per_meta)
    cls = rng.integers(0, 13, size=q.size)
    cell = rng.integers(0, 648, size=q.size)
    side = (cell // 36) * 36 + (cell % 36 + 1) % 36
    f = table.first[q][:, None] + np.arange(5)[None, :]                            # [E, 5] frames, some past the length
    live = np.arange(5)[None, :] < table.length[q][:, None]
    for back in range(5):                                                          # the up-to-5 windows covering a frame
        w = f // 50 - back
        ok = live & (w >= 0) & (w < n_w)
        e, _ = np.nonzero(ok)
        wi, ti = (torch.from_numpy(a[ok]).to(device) for a in (w, f - 50 * w))
        ci = torch.from_numpy(cls[e]).to(device)
        for target, gain in ((cell, 8.0), (side, 6.0)):
            xi = torch.from_numpy(target[e]).to(device)
            logits[wi, ti, xi, ci] = (logits[wi, ti, xi, ci].float() + gain).to(logits.dtype)
    return int(q.size)


def worker(args):
    """One profiled process: `passes` + 1 rounds over the timeline (the first is the warm-up), the candidates this
    package has taking turns inside every round."""
    import numpy as np
    import torch
    sys.path.insert(0, str(Path(args.package).resolve()))
    import seld_eval
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
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
    planted = plant_sources(logits, table, np.random.default_rng(11), device)
    k, q_n, b = 4, len(table), args.batch
    det = (torch.empty((q_n, 13, k), dtype=torch.int32, device=device),
           torch.empty((q_n, 13, k), dtype=torch.float32, device=device),
           torch.empty((q_n, 13), dtype=torch.int32, device=device),
           torch.empty((q_n, 13, k, 2), dtype=torch.float32, device=device))
    plan, done = [], 0                          # (w0, w1, q0, q1) of each streaming step
    for lo in range(0, n_w, b):
        hi = min(lo + b, n_w)
        end = int(np.searchsorted(table.last_window, hi - 1, side="right"))
        plan.append((max(0, lo - seld_eval.KEEP_WINDOWS), hi, done, end))
        done = end
    refine = hasattr(seld_eval, "grid_decode_refine")
    rng = np.random.default_rng(7)
    rows = [np.array(synthetic_rows(rng, frames), dtype=np.int64).reshape(-1, 5) for _ in range(args.clips)]
    offsets, dirs = seld_eval.reference_table(table, rows)
    offsets_d, dirs_d = torch.from_numpy(offsets).to(device), torch.from_numpy(dirs).to(device)
    for _ in range(args.passes + 1):
        for w0, w1, q0, q1 in plan:
            if q1 > q0:
                seld_eval.grid_decode(logits[w0:w1], w0, table, q0, q1 - q0, 0.5, k, out=tuple(t[q0:q1] for t in det[:3]))
        if refine:
            for w0, w1, q0, q1 in plan:
                if q1 > q0:
                    seld_eval.grid_decode_refine(logits[w0:w1], w0, table, q0, q1 - q0, 0.5, k,
                                                 out=tuple(t[q0:q1] for t in det))
        seld_eval.doa_match(det[0], det[2], offsets_d, dirs_d, 20.0)
        if refine:
            seld_eval.doa_match_dirs(det[3], det[2], offsets_d, dirs_d, 20.0)
    torch.cuda.synchronize()
    print(json.dumps({"windows": n_w, "meta_frames": q_n, "calls_per_pass": sum(q1 > q0 for _, _, q0, q1 in plan),
                      "planted": planted, "detections": int(det[2].sum()), "references": int(offsets[-1]), "refine": refine}), flush=True)


def profiled(args, package, directory):
    """Run the worker on ``package`` under rocprofv3; {candidate: median launch in us, warm-up pass dropped}."""
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "-f", "csv", "-d", str(directory), "--", sys.executable,
           str(Path(__file__).resolve()), "--worker", "--package", str(package), "--clips", str(args.clips), "--seconds",
           str(args.seconds), "--batch", str(args.batch), "--passes", str(args.passes)]
    run = subprocess.run(cmd, capture_output=True, text=True, timeout=args.timeout)
    if run.returncode != 0:
        raise RuntimeError(f"{' '.join(cmd)} failed with {run.returncode}:\n{run.stdout[-2000:]}\n{run.stderr[-4000:]}")
    info = json.loads([line for line in run.stdout.splitlines() if line.startswith("{")][-1])
    traces = list(Path(directory).rglob("*kernel_trace.csv"))
    if len(traces) != 1:
        raise RuntimeError(f"expected one kernel trace under {directory}, found {traces}")
    return parse_trace(traces[0], args.passes), info


def parse_trace(path, passes):
    """kernel_trace.csv of one worker -> {candidate: median launch duration in us over the timed passes}."""
    launches = {}
    with open(path, newline="") as fh:
        for r in csv.DictReader(fh):
            for needle, name in KERNELS:
                if needle in r["Kernel_Name"]:
                    launches.setdefault(name, []).append((int(r["Start_Timestamp"]), int(r["End_Timestamp"])))
                    break
    out = {}
    for name, rows in launches.items():
        rows.sort()
        per_pass = len(rows) // (passes + 1)
        out[name] = statistics.median((e - s) / 1e3 for s, e in rows[per_pass:])
    return out


def summary(samples):
    return {"median_us": statistics.median(samples), "min_us": min(samples), "max_us": max(samples),
            "spread_us": max(samples) - min(samples), "samples_us": samples}


def main():
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--clips", type=int, default=32)
    p.add_argument("--seconds", type=int, default=60)
    p.add_argument("--batch", type=int, default=16)
    p.add_argument("--passes", type=int, default=3, help="timed rounds over the timeline per process, after one warm-up")
    p.add_argument("--samples", type=int, default=5, help="profiled processes per side")
    p.add_argument("--timeout", type=int, default=300, help="seconds allowed to one profiled process")
    p.add_argument("--parent-package", default=None,
                   help="the parent commit's sound-event-localization-detection_amd directory, built (the yardstick)")
    p.add_argument("--package", default=str(PACKAGE), help=argparse.SUPPRESS)
    p.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    p.add_argument("--out", default=None)
    args = p.parse_args()
    if args.worker:
        return worker(args)
    samples = {"parent": {}, "this": {}}
    info = {}
    with tempfile.TemporaryDirectory() as tmp:
        for s in range(args.samples):
            for side, package in (("parent", args.parent_package), ("this", PACKAGE)):
                if package is None:
                    continue
                got, info[side] = profiled(args, package, Path(tmp) / f"{side}{s}")
                for name, us in got.items():
                    samples[side].setdefault(name, []).append(us)
                print(json.dumps({"sample": s, "side": side, **got}), flush=True)
    out = {"workload": {"clips": args.clips, "seconds": args.seconds, "batch": args.batch, "max_peaks": 4,
                        "passes": args.passes, "samples": args.samples, **info.get("this", {})},
           "unit": "median kernel duration per launch, microseconds (rocprofv3 --kernel-trace)",
           "this_tree": {name: summary(v) for name, v in samples["this"].items()},
           "parent": {name: summary(v) for name, v in samples["parent"].items()}}
    this, parent = out["this_tree"], out["parent"]
    if "plain_decode" in parent:
        base = parent["plain_decode"]
        out["refined_minus_parent_plain_us"] = this["refined_decode"]["median_us"] - base["median_us"]
        out["plain_minus_parent_plain_us"] = this["plain_decode"]["median_us"] - base["median_us"]
        out["parent_plain_spread_us"] = base["spread_us"]
        out["refined_exceeds_parent_spread"] = out["refined_minus_parent_plain_us"] > base["spread_us"]
    out["match_dirs_minus_match_us"] = this["match_dirs"]["median_us"] - this["match"]["median_us"]
    print(json.dumps({k: v for k, v in out.items() if not isinstance(v, dict)}), flush=True)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(out, indent=2) + "\n")


if __name__ == "__main__":
    main()
