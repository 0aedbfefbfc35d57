"""Developer experiment: forward of encoder blocks 2-4 up to the pooled output (bf16, channels-last, B = 32, T = 250),
HIP events -- the library convolution followed by the tail with its statistics pass (F.conv2d + tail_stats_kernel +
finalise + apply) against csrc/convfwd.hip with the statistics epilogue followed by finalise + apply.  Both sides end
with the same finalise and apply launches, so the difference of the two is (library convolution + tail_stats_kernel)
against (own kernel with statistics); the convolutions alone are reported beside them.

The sides alternate, SAMPLES samples each (a sample = REPS back-to-back calls between two events).  Adoption rule: a
block uses the own kernel only if its slowest sample is faster than the library side's fastest one."""
import sys
from pathlib import Path
ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "sound-event-localization-detection_amd")]
import torch
import torch.nn.functional as F
import seld_native
torch.backends.cudnn.benchmark = True
dev = torch.device("cuda:0")
SAMPLES, REPS, WARM = 7, 20, 5


def sample(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(REPS):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / REPS * 1e3


cl = torch.channels_last
for block, (cin, cout, f) in enumerate(((64, 128, 32), (128, 256, 16), (256, 512, 8)), start=2):
    w = (torch.randn(cout, cin, 3, 3, device=dev) * 0.05).to(torch.bfloat16).contiguous(memory_format=cl)
    x = torch.randn(32, cin, 250, f, device=dev).to(torch.bfloat16).contiguous(memory_format=cl)
    gamma, beta = torch.rand(cout, device=dev) + 0.5, torch.randn(cout, device=dev)
    rm, rv = torch.zeros(cout, device=dev), torch.ones(cout, device=dev)
    gflop = 2.0 * cout * 9 * cin * 32 * 250 * f / 1e9
    assert seld_native.conv3x3_forward_applicable(x, w)

    def library():
        y = F.conv2d(x, w, padding=1)
        return seld_native.conv_tail_forward(y, gamma, beta, rm, rv, 0.1, 1e-5, True, 2)[0]

    def own():
        y, partials = seld_native.conv3x3_forward(x, w, stats=True)
        return seld_native.conv_tail_forward_from_partials(y, partials, gamma, beta, rm, rv, 0.1, 1e-5, 2)[0]

    sides = {"conv": lambda: F.conv2d(x, w, padding=1),
             "own conv": lambda: seld_native.conv3x3_forward(x, w),
             "own+sums": lambda: seld_native.conv3x3_forward(x, w, stats=True),
             "library": library,
             "own": own}
    for fn in sides.values():
        for _ in range(WARM):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in sides}
    for _ in range(SAMPLES):
        for k, fn in sides.items():
            times[k].append(sample(fn))
    ref = F.conv2d(x.float(), w.float(), padding=1)
    got = seld_native.conv3x3_forward(x, w)
    diff = (got.float() - ref).abs().max().item() / ref.abs().max().item()
    med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
    adopt = max(times["own"]) < min(times["library"])
    print(f"block {block}: {cin:3d}->{cout:3d} F={f:2d} ({gflop:6.1f} GFLOP)", flush=True)
    for k in sides:
        rate = f" ({gflop / med[k] * 1e3:6.0f} TFLOP/s)" if k in ("conv", "own conv", "own+sums") else ""
        print(f"    {k:8s} median {med[k]:7.1f} us  min {min(times[k]):7.1f}  max {max(times[k]):7.1f}{rate}", flush=True)
    print(f"    own vs fp32 library result: max abs diff / max |ref| {diff:.1e}; "
          f"own slowest {max(times['own']):.1f} us vs library fastest {min(times['library']):.1f} us -> "
          f"{'ADOPT the own kernel' if adopt else 'KEEP the library'}", flush=True)
