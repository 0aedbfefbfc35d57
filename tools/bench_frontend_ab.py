"""This tree's library and another build in ONE process, sides alternating, HIP events (the method of
tools/bench_bf16_helper_ab.py): the three front-end rows of bench.py's kernel table -- log-mel of 8 clips x 4 ch of int16
PCM, ``spatial_features`` logmel_gcc of 8 clips x 8 ch and logmel_iv of 8 clips x 4 ch -- with stft and logmel_nipd at
the same size, and gru_forward / gru_backward at B = 32, T = 250 (their launchers take the dynamic-LDS opt-in from the
same helper).    python tools/bench_frontend_ab.py PARENT_LIBSELD_HIP.so"""
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

os.environ["SELD_HIP_LIB"] = sys.argv[1]
spec = importlib.util.spec_from_file_location("seld_native_parent", PKG / "seld_native.py")
parent = importlib.util.module_from_spec(spec)
spec.loader.exec_module(parent)
assert parent.LIB_PATH != seld_native.LIB_PATH
dev = torch.device("cuda:0")
SAMPLES, WARM = 11, 3
CLIPS, CLIP_SAMPLES, BATCH, WINDOW, H = 8, 24000 * 60, 32, 250, 256
MODS = {"parent": parent, "tree": seld_native}
print(f"this tree {seld_native.LIB_PATH}\nparent    {parent.LIB_PATH}\n{SAMPLES} alternating samples of back-to-back calls, us per call",
      flush=True)


def sample(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3


def ab(name, make, reps):
    sides = {k: make(m) for k, m in MODS.items()}
    for fn in sides.values():
        for _ in range(WARM):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in sides}
    for _ in range(SAMPLES):
        for k, fn in sides.items():
            times[k].append(sample(fn, reps))
    p, t = sorted(times["parent"]), sorted(times["tree"])
    mp, mt = statistics.median(p), statistics.median(t)
    print(f"{name}: parent median {mp:.1f} ({p[0]:.1f} - {p[-1]:.1f}, spread {p[-1] - p[0]:.1f})  tree median {mt:.1f} "
          f"({t[0]:.1f} - {t[-1]:.1f})  tree - parent {mt - mp:+.1f}  inside the parent's spread: {mt - mp <= p[-1] - p[0]}",
          flush=True)


torch.manual_seed(0)
pcm16 = (torch.randn(CLIPS, 4, CLIP_SAMPLES, device=dev) * 3276.8).clamp(-32768, 32767).to(torch.int16)
lm_out = torch.empty(CLIPS, 1 + CLIP_SAMPLES // 480, 4, 64, device=dev)
ab(f"logmel {CLIPS} clips x 4 ch int16", lambda m: lambda: m.logmel(pcm16, layout="tcf", out=lm_out), 5)
del pcm16, lm_out
pcm8 = torch.randn(CLIPS, 8, CLIP_SAMPLES, device=dev) * 0.1
ab(f"spatial_features logmel_gcc {CLIPS} clips x 8 ch", lambda m: lambda: m.spatial_features(pcm8, "logmel_gcc"), 3)
ab(f"spatial_features logmel_nipd {CLIPS} clips x 8 ch", lambda m: lambda: m.spatial_features(pcm8, "logmel_nipd"), 3)
del pcm8
pcm4 = torch.randn(CLIPS, 4, CLIP_SAMPLES, device=dev) * 0.1
ab(f"spatial_features logmel_iv {CLIPS} clips x 4 ch", lambda m: lambda: m.spatial_features(pcm4, "logmel_iv"), 3)
ab(f"stft {CLIPS} clips x 4 ch", lambda m: lambda: m.stft(pcm4), 3)
del pcm4
torch.cuda.empty_cache()

gi = (torch.randn(BATCH, WINDOW, 2, 3 * H, device=dev) * 0.5).to(torch.bfloat16)
w_hh = torch.randn(2, 3 * H, H, device=dev) * 0.05
b_hn = torch.zeros(2, H, device=dev)
dy = torch.randn(BATCH, WINDOW, 2 * H, device=dev).to(torch.bfloat16)
y, saved = seld_native.gru_forward(gi, w_hh, b_hn, True)
ab(f"gru_forward B = {BATCH}, T = {WINDOW}", lambda m: lambda: m.gru_forward(gi, w_hh, b_hn, True), 10)
ab(f"gru_backward B = {BATCH}, T = {WINDOW}", lambda m: lambda: m.gru_backward(dy, saved, y, w_hh), 10)
