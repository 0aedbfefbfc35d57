"""This tree's library and another build in ONE process, sides alternating, HIP events (the method of
tools/bench_conv_loop_ab.py): LayerNorm forward / backward (bf16, D = 512, with and without ReLU) and multi_adam /
multi_adam_guarded at the CRNN's parameter count.    python tools/bench_bf16_helper_ab.py PARENT_LIBSELD_HIP.so"""
import importlib.util
import os
import statistics
import sys
from pathlib import Path
ROOT = Path(__file__).resolve().parent.parent
PKG = ROOT / "sound-event-localization-detection_amd"
sys.path[:0] = [str(ROOT), str(PKG)]
import torch
import seld_native
import trainer

os.environ["SELD_HIP_LIB"] = sys.argv[1]
spec = importlib.util.spec_from_file_location("seld_native_parent", PKG / "seld_native.py")
parent = importlib.util.module_from_spec(spec)
spec.loader.exec_module(parent)
assert parent.LIB_PATH != seld_native.LIB_PATH
dev = torch.device("cuda:0")
SAMPLES, REPS, WARM = 11, 50, 10
print(f"this tree {seld_native.LIB_PATH}\nparent    {parent.LIB_PATH}\n{SAMPLES} alternating samples of {REPS} back-to-back calls, us per call", flush=True)


def sample(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(REPS):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / REPS * 1e3


def ab(name, sides):
    for fn in sides.values():
        for _ in range(WARM):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in sides}
    for _ in range(SAMPLES):
        for k, fn in sides.items():
            times[k].append(sample(fn))
    p, t = sorted(times["parent"]), sorted(times["tree"])
    mp, mt = statistics.median(p), statistics.median(t)
    print(f"{name}: parent median {mp:.2f} ({p[0]:.2f} - {p[-1]:.2f}, spread {p[-1] - p[0]:.2f})  tree median {mt:.2f} "
          f"({t[0]:.2f} - {t[-1]:.2f})  tree - parent {mt - mp:+.2f}  inside the parent's spread: {mt - mp <= p[-1] - p[0]}", flush=True)


torch.manual_seed(0)
rows, d = 32 * 250, 512
x = torch.randn(rows, d, device=dev).to(torch.bfloat16)
dy = torch.randn(rows, d, device=dev).to(torch.bfloat16)
w, b = torch.randn(d, device=dev), torch.randn(d, device=dev)
y, stats = seld_native.layernorm_forward(x, w, b, 1e-5, False)
parent.layernorm_forward(x, w, b, 1e-5, False)                       # initialises the other library's device state
dx, dwt, dbs = torch.empty_like(x), torch.empty(d, device=dev), torch.empty(d, device=dev)
P, st = seld_native._p, seld_native._stream_ptr(dev)
libs = {"parent": parent.load_library(), "tree": seld_native.load_library()}
ws = torch.empty(int(libs["tree"].seld_layernorm_workspace_floats(rows, d)), device=dev)
for relu in (0, 1):
    ab(f"layernorm_forward bf16 8000x512 relu={relu}",
       {k: (lambda lib=lib: lib.seld_layernorm_forward(P(x), 1, rows, d, P(w), P(b), 1e-5, relu, P(y), P(stats), st))
        for k, lib in libs.items()})
    ab(f"layernorm_backward bf16 8000x512 relu={relu} (backward + final kernel)",
       {k: (lambda lib=lib: lib.seld_layernorm_backward(P(x), P(dy), 1, rows, d, P(w), P(b), P(stats), relu, P(dx), P(dwt),
                                                        P(dbs), P(ws), st)) for k, lib in libs.items()})

trainer.config.MODEL_TYPE = "crnn"
model = trainer.build_model((18, 36))
params = [p.detach().float().to(dev).contiguous() for p in model.parameters()]
grads = [torch.randn_like(p).to(torch.bfloat16 if p.dim() >= 2 else torch.float32) * 1e-3 for p in params]
ms = [torch.zeros_like(p) for p in params]
vs = [torch.zeros_like(p) for p in params]
lows = [p.to(torch.bfloat16) if p.dim() >= 2 else None for p in params]
lr, step = torch.full((1,), 1e-3, device=dev), torch.ones(1, device=dev)
mods = {"parent": parent, "tree": seld_native}
caches = {k: {} for k in mods}
ab(f"multi_adam {len(params)} tensors {sum(p.numel() for p in params)} elements",
   {k: (lambda m=m, k=k: m.multi_adam(grads, params, ms, vs, lows, lr, step, 0.9, 0.999, 1e-8, 0.0, cache=caches[k]))
    for k, m in mods.items()})
caches = {k: {} for k in mods}
ab("multi_adam_guarded (no guard record, no EMA)",
   {k: (lambda m=m, k=k: m.multi_adam_guarded(grads, params, ms, vs, lows, lr, step, 0.9, 0.999, 1e-8, 0.0, cache=caches[k]))
    for k, m in mods.items()})
srcs = [p for p in params if p.dim() >= 2]
dsts = [torch.empty_like(p, dtype=torch.bfloat16) for p in srcs]
caches = {k: {} for k in mods}
ab(f"multi_cast fp32 -> bf16, {len(srcs)} tensors",
   {k: (lambda m=m, k=k: m.multi_cast(srcs, dsts, cache=caches[k])) for k, m in mods.items()})
