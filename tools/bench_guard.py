#!/usr/bin/env python
"""Cost of the guarded optimiser update (csrc/guard.hip + the guarded instantiation of csrc/adam.hip; DESIGN.md section
12), on the GPU.

  python tools/bench_guard.py                      kernels + end to end, one JSON document (also --out FILE)
  python tools/bench_guard.py --skip-e2e           kernels only

Kernels, on the REAL parameter lists of the full-size CRNN and the ResNet50-Conformer in the master-weight arrangement (bf16
working weights with bf16 gradients + the fp32 rest): seld_multi_adam against seld_multi_grad_norm + seld_multi_adam_guarded,
without and with the weight EMA, alternating in one process.  A timed sample is a burst of updates captured as one HIP graph
and replayed between two device events (an update is a few launches of microseconds each: an eager loop would time the
host).  Bytes are the algorithm's: 28 B per parameter for Adam, + the gradient once more for the norm (2 or
4 B), + 8 B for the EMA.  The parameter sets (tens of MB) fit the Infinity Cache, as they do in training.

End to end: full-size CRNN, batch 32, captured training steps, guard off / on (clipping + skip + EMA) in alternating rounds;
two models and two steppers in one process, fed the same batch.
"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
for p in (str(ROOT), str(ROOT / "sound-event-localization-detection_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

HBM_PEAK = 8.0e12
B = 32


class Burst:
    def __init__(self, fn, n):
        self.n = n
        fn()
        fn()
        torch.cuda.synchronize()
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            for _ in range(n):
                fn()
        self.e0, self.e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def us(self):
        self.e0.record()
        self.graph.replay()
        self.e1.record()
        self.e1.synchronize()
        return self.e0.elapsed_time(self.e1) * 1e3 / self.n


def parameter_lists(kind, dev):
    import trainer
    cfg = trainer.config
    saved = cfg.MODEL_TYPE
    cfg.MODEL_TYPE = kind
    try:
        torch.manual_seed(0)
        model = trainer.prepare_model_for_device(trainer.build_model((18, 36)), dev)
        trainer.enable_master_weights(model, dev)
        low, masters, _ = trainer.unwrap(model)._seld_master_weights
        low_ids = {id(p) for p in low}
        others = [p for p in model.parameters() if id(p) not in low_ids]
        return model, low, masters, others
    finally:
        cfg.MODEL_TYPE = saved


def bench_kernels(dev, kind, bursts, burst_len):
    import seld_native as nat
    model, low, masters, others = parameter_lists(kind, dev)
    params = list(masters) + [p.data for p in others]
    grads = [torch.randn_like(p.data) * 0.01 for p in low] + [torch.randn_like(p.data) * 0.01 for p in others]
    lows = [p.data for p in low] + [None] * len(others)
    m = [torch.zeros_like(p) for p in params]
    v = [torch.zeros_like(p) for p in params]
    ema = [p.clone() for p in params]
    lr = torch.tensor(1e-4, device=dev)
    step = torch.tensor(100.0, device=dev)
    guard = nat.new_guard_record(dev)
    partial = torch.zeros(nat.grad_norm_scratch_floats([p.numel() for p in params]), device=dev)
    caches = [{} for _ in range(5)]
    n_bf16, n_fp32 = sum(p.numel() for p in low), sum(p.numel() for p in others)
    adam_bytes = 28 * (n_bf16 + n_fp32)          # bf16 gradient 2 + 12 read, 12 + 2 (working copy) written; fp32: 4 + 12, 12
    norm_bytes = 2 * n_bf16 + 4 * n_fp32
    ema_bytes = 8 * (n_bf16 + n_fp32)
    args = (0.9, 0.999, 1e-8, 1e-4)

    def plain():
        assert nat.multi_adam(grads, params, m, v, lows, lr, step, *args, 1.0, caches[0])

    def guarded():
        assert nat.multi_grad_norm(grads, guard, partial, 1.0, 1.0, True, caches[1])
        assert nat.multi_adam_guarded(grads, params, m, v, lows, lr, step, *args, 1.0, None, 0.0, guard, caches[2])

    def guarded_ema():
        assert nat.multi_grad_norm(grads, guard, partial, 1.0, 1.0, True, caches[1])
        assert nat.multi_adam_guarded(grads, params, m, v, lows, lr, step, *args, 1.0, ema, 0.999, guard, caches[3])

    def norm_only():
        assert nat.multi_grad_norm(grads, guard, partial, 1.0, 1.0, True, caches[1])

    sides = {"multi_adam": (plain, adam_bytes), "grad_norm": (norm_only, norm_bytes),
             "grad_norm+adam_guarded": (guarded, adam_bytes + norm_bytes),
             "grad_norm+adam_guarded+ema": (guarded_ema, adam_bytes + norm_bytes + ema_bytes)}
    runs = {k: Burst(fn, burst_len) for k, (fn, _) in sides.items()}
    for r in runs.values():
        r.us()
    samples = {k: [] for k in sides}
    for _ in range(bursts):                                       # alternate the sides inside every round
        for k, r in runs.items():
            samples[k].append(r.us())
    out = {"model": kind, "tensors": len(params), "launches_adam": (len(params) + 47) // 48,
           "launches_norm": (len(params) + 47) // 48 + 1, "parameters_bf16_grad": n_bf16, "parameters_fp32_grad": n_fp32,
           "bursts": bursts, "updates_per_burst": burst_len, "sides": {}}
    for k, vals in samples.items():
        med = statistics.median(vals)
        nbytes = sides[k][1]
        out["sides"][k] = {"us_median": round(med, 2), "us_min": round(min(vals), 2), "us_max": round(max(vals), 2),
                           "algorithmic_bytes": nbytes, "share_of_8TBps": round(nbytes / (med * 1e-6) / HBM_PEAK, 4)}
    base = out["sides"]["multi_adam"]["us_median"]
    out["guard_extra_us"] = round(out["sides"]["grad_norm+adam_guarded"]["us_median"] - base, 2)
    out["guard_ema_extra_us"] = round(out["sides"]["grad_norm+adam_guarded+ema"]["us_median"] - base, 2)
    return out


def bench_end_to_end(dev, rounds, steps):
    import trainer
    cfg = trainer.config
    keys = ("MODEL_TYPE", "GRAD_CLIP_NORM", "SKIP_NONFINITE_STEPS", "EMA_DECAY")
    saved = {k: getattr(cfg, k) for k in keys}
    cfg.MODEL_TYPE = "crnn"
    try:
        g = torch.Generator().manual_seed(0)
        spec = (torch.randn(B, 250, 4, 64, generator=g) * 20 - 30).to(dev)
        mask = ((torch.rand(B, 250, 648, generator=g) < 0.02).to(torch.int32) << 3).to(torch.uint16).to(dev)
        weights = torch.ones(14, device=dev)
        weights[13] = 0.05
        steppers, opts = {}, {}
        for on in (False, True):
            cfg.GRAD_CLIP_NORM, cfg.SKIP_NONFINITE_STEPS, cfg.EMA_DECAY = (1.0, True, 0.999) if on else (0.0, False, 0.0)
            torch.manual_seed(0)
            model = trainer.prepare_model_for_device(trainer.build_model((18, 36)), dev).train()
            trainer.enable_master_weights(model, dev)
            crit = trainer.SMRSELDLoss(loss_type="mse", w_class=1.0, grid_size=(18, 36), class_weights=weights)
            opt = trainer.make_optimizer(model, cfg.LEARNING_RATE, dev, capturable=True)
            steppers[on], opts[on] = trainer.make_stepper(model, crit, opt, dev, 1), opt

        def run(on):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                steppers[on](spec, mask)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3 / steps

        for on in (False, True, False, True):                       # warm-ups + capture of both
            run(on)
        off, onn = [], []
        for _ in range(rounds):
            off.append(run(False))
            onn.append(run(True))
        report = opts[True].guard_report()
        stats = {on: steppers[on].stats() for on in steppers}
        for s in steppers.values():
            s.close()
        med_off, med_on = statistics.median(off), statistics.median(onn)
        spread = max(max(off) - min(off), max(onn) - min(onn))
        return {"model": "crnn", "batch": B, "rounds": rounds, "steps_per_round": steps,
                "guard_on": {"GRAD_CLIP_NORM": 1.0, "SKIP_NONFINITE_STEPS": True, "EMA_DECAY": 0.999},
                "captured": {str(on): stats[on]["graphs"] for on in stats}, "guard_report": report,
                "ms_per_step_off": [round(x, 4) for x in off], "ms_per_step_on": [round(x, 4) for x in onn],
                "median_off_ms": round(med_off, 4), "median_on_ms": round(med_on, 4),
                "on_minus_off_ms": round(med_on - med_off, 4), "on_over_off": round(med_on / med_off, 5),
                "spread_ms": round(spread, 4), "difference_inside_spread": bool(abs(med_on - med_off) <= spread)}
    finally:
        for k, val in saved.items():
            setattr(cfg, k, val)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None)
    ap.add_argument("--bursts", type=int, default=30)
    ap.add_argument("--burst-len", type=int, default=10)
    ap.add_argument("--skip-e2e", action="store_true")
    ap.add_argument("--e2e-rounds", type=int, default=8)
    ap.add_argument("--e2e-steps", type=int, default=12)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_guard.py measures on the GPU: no ROCm device visible")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    doc = {"kernels": [bench_kernels(dev, kind, args.bursts, args.burst_len) for kind in ("crnn", "resnet_conformer")]}
    doc["end_to_end"] = None if args.skip_e2e else bench_end_to_end(dev, args.e2e_rounds, args.e2e_steps)
    text = json.dumps(doc, indent=1)
    print(text)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
