"""Developer experiment: data gradient of the encoder's 3x3 convolutions alone (bf16, channels-last, B = 32, T = 250),
HIP events -- the library path of model_crnn._Conv3x3.backward (seld_native.conv_weight_flip_transpose + a forward
F.conv2d of dy with the transformed weights) against csrc/convdgrad.hip (one launch, the weights read where they lie).

The two sides alternate, SAMPLES samples each (a sample = REPS back-to-back calls between two events).  Adoption rule:
a block uses the own kernel only if the kernel's slowest sample is faster than the library path's fastest one."""
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
    dy = torch.randn(32, cout, 250, f, device=dev).to(torch.bfloat16).contiguous(memory_format=cl)
    gflop = 2.0 * cout * 9 * cin * 32 * 250 * f / 1e9
    assert seld_native.conv3x3_dgrad_applicable(dy, w)
    wt = seld_native.conv_weight_flip_transpose(w)
    sides = {"flip": lambda: seld_native.conv_weight_flip_transpose(w),
             "conv": lambda: F.conv2d(dy, wt, padding=1),
             "library": lambda: F.conv2d(dy, seld_native.conv_weight_flip_transpose(w), padding=1),
             "own": lambda: seld_native.conv3x3_dgrad(dy, w)}
    for fn in sides.values():
        for _ in range(WARM):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in sides}
    for _ in range(SAMPLES):
        for k, fn in sides.items():
            times[k].append(sample(fn))
    ref = F.conv2d(dy.float(), wt.float(), padding=1)
    got = seld_native.conv3x3_dgrad(dy, w)
    diff = (got.float() - ref).abs().max().item() / ref.abs().max().item()
    med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
    adopt = max(times["own"]) < min(times["library"])
    print(f"block {block}: {cout:3d}->{cin:3d} F={f:2d} ({gflop:6.1f} GFLOP)", flush=True)
    for k in sides:
        rate = f" ({gflop / med[k] * 1e3:6.0f} TFLOP/s)" if k != "flip" else ""
        print(f"    {k:8s} median {med[k]:7.1f} us  min {min(times[k]):7.1f}  max {max(times[k]):7.1f}{rate}", flush=True)
    print(f"    own vs fp32 library result: max abs diff / max |ref| {diff:.1e}; "
          f"own slowest {max(times['own']):.1f} us vs library fastest {min(times['library']):.1f} us -> "
          f"{'ADOPT the own kernel' if adopt else 'KEEP the library'}", flush=True)
