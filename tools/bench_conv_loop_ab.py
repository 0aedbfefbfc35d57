"""Developer experiment: the six launches of the flagship iteration that run csrc/conv3x3_loop.h (forward with the
statistics epilogue and data gradient of encoder blocks 2-4; bf16, channels-last, B = 32, T = 250), this tree's build
against another build of the library in one process, HIP events.

    python tools/bench_conv_loop_ab.py PARENT_LIBSELD_HIP.so

The two sides alternate, SAMPLES samples each (a sample = REPS back-to-back calls between two events).  Adoption rule:
a launch keeps the new schedule only if this tree's slowest sample is faster than the other build's fastest one.  The
results of the two builds are compared bit for bit as well."""
import importlib.util
import os
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
assert parent.LIB_PATH != seld_native.LIB_PATH, (parent.LIB_PATH, seld_native.LIB_PATH)
dev = torch.device("cuda:0")
SAMPLES, REPS, WARM = 9, 20, 5


def sample(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(REPS):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / REPS * 1e3


cl = torch.channels_last
print(f"this tree {seld_native.LIB_PATH}\nparent    {parent.LIB_PATH}", flush=True)
for block, (cin, cout, f) in enumerate(((64, 128, 32), (128, 256, 16), (256, 512, 8)), start=2):
    w = (torch.randn(cout, cin, 3, 3, device=dev) * 0.05).to(torch.bfloat16).contiguous(memory_format=cl)
    x = torch.randn(32, cin, 250, f, device=dev).to(torch.bfloat16).contiguous(memory_format=cl)
    dy = torch.randn(32, cout, 250, f, device=dev).to(torch.bfloat16).contiguous(memory_format=cl)
    gflop = 2.0 * cout * 9 * cin * 32 * 250 * f / 1e9
    y, dx = torch.empty_like(dy), torch.empty_like(x)
    partials = torch.empty(2, seld_native.conv3x3_forward_chunks(32, 250, f), cout, device=dev)
    for name, sides in (("forward+sums", {"parent": lambda: parent.conv3x3_forward(x, w, stats=True, out=y, partials=partials),
                                          "tree": lambda: seld_native.conv3x3_forward(x, w, stats=True, out=y, partials=partials)}),
                        ("data gradient", {"parent": lambda: parent.conv3x3_dgrad(dy, w, out=dx),
                                           "tree": lambda: seld_native.conv3x3_dgrad(dy, w, out=dx)})):
        results = {}
        for k, fn in sides.items():
            for _ in range(WARM):
                fn()
            torch.cuda.synchronize()
            r = fn()
            results[k] = [v.clone() for v in (r if isinstance(r, tuple) else (r,))]
        same = all(torch.equal(a, b) for a, b in zip(results["parent"], results["tree"]))
        times = {k: [] for k in sides}
        for _ in range(SAMPLES):
            for k, fn in sides.items():
                times[k].append(sample(fn))
        med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
        keep = max(times["tree"]) < min(times["parent"])
        print(f"block {block} {name:13s} ({gflop:6.1f} GFLOP)  bits {'identical' if same else 'DIFFER'}", flush=True)
        for k in sides:
            print(f"    {k:6s} median {med[k]:7.1f} us  min {min(times[k]):7.1f}  max {max(times[k]):7.1f} "
                  f"({gflop / med[k] * 1e3:6.0f} TFLOP/s)", flush=True)
        print(f"    tree slowest {max(times['tree']):.1f} us vs parent fastest {min(times['parent']):.1f} us -> "
              f"{'NEW schedule' if keep else 'KEEP the parent schedule'} ({(med['tree'] / med['parent'] - 1) * 100:+.1f} % kernel time)",
              flush=True)
