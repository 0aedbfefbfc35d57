"""Developer experiment: weight gradient of the encoder's 3x3 convolutions alone (bf16, channels-last, B = 32,
T = 250), HIP events -- the library's backward-weight solver (plus the cast into a bf16 gradient it needs) against
csrc/convwgrad.hip (split-K MFMA kernel + fixed-order slab sum, written straight into the bf16 gradient)."""
import sys
from pathlib import Path
ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "sound-event-localization-detection_amd")]
import torch
import seld_native
torch.backends.cudnn.benchmark = True
dev = torch.device("cuda:0")


def timeit(fn, reps=20, warm=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3


cl = torch.channels_last
for cin, cout, f in ((4, 64, 64), (64, 128, 32), (128, 256, 16), (256, 512, 8)):
    x = torch.randn(32, cin, 250, f, device=dev).to(torch.bfloat16).contiguous(memory_format=cl)
    w = (torch.randn(cout, cin, 3, 3, device=dev) * 0.05).to(torch.bfloat16).contiguous(memory_format=cl)
    dy = torch.randn(32, cout, 250, f, device=dev).to(torch.bfloat16).contiguous(memory_format=cl)
    dw = torch.empty_like(w)
    gflop = 2.0 * cout * 9 * cin * 32 * 250 * f / 1e9

    def library():
        dw.copy_(torch.ops.aten.convolution_backward(dy, x, w, None, (1, 1), (1, 1), (1, 1), False, (0, 0), 1,
                                                     (False, True, False))[1])
    t_lib = timeit(library)
    line = f"{cin:3d}->{cout:3d} F={f:2d} ({gflop:6.1f} GFLOP): library {t_lib:7.1f} us ({gflop / t_lib * 1e3:6.0f} TFLOP/s)"
    if seld_native.conv3x3_wgrad_applicable(x, dy, w):
        t_own = timeit(lambda: seld_native.conv3x3_wgrad(x, dy, dw))
        ref = torch.ops.aten.convolution_backward(dy.float(), x.float(), w.float(), None, (1, 1), (1, 1), (1, 1),
                                                  False, (0, 0), 1, (False, True, False))[1]
        seld_native.conv3x3_wgrad(x, dy, dw)
        err = (dw.float() - ref).abs().max().item() / ref.abs().max().item()
        line += f" | convwgrad {t_own:7.1f} us ({gflop / t_own * 1e3:6.0f} TFLOP/s, rel diff {err:.1e})"
    print(line, flush=True)
