"""Developer experiment: the encoder's first block alone at the bench's shape (B = 32, 4 -> 64 channels, T = 250, F = 64,
bf16 channels-last), HIP events after warm-up -- each kernel of csrc/convfirst.hip on its own against the launches of
the general path it replaces (library convolution, seld_conv_tail_forward / backward, library weight gradient with the
copy into a bf16 gradient), with the HBM bytes each side has to move set against the 6.3 TB/s copy rate."""
import sys
from pathlib import Path
ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "sound-event-localization-detection_amd")]
import torch
import torch.nn.functional as F
import seld_native
torch.backends.cudnn.benchmark = True
dev = torch.device("cuda:0")
COPY_RATE = 6.3e12


def timeit(fn, reps=20, warm=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    # hold the stream (3 x 1 ms) while the host enqueues the repetitions: the events then bracket back-to-back kernels,
    # not the Python / ctypes time per call that exceeds the small ones (bench.py's timeit)
    for _ in range(3):
        seld_native.stream_delay(dev, 1_000_000)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3


def line(name, us, mbytes):
    floor = mbytes * 1e6 / COPY_RATE * 1e6
    print(f"  {name:<46s} {us:7.1f} us   {mbytes:6.1f} MB  ({floor:5.1f} us at the copy rate, {mbytes / us:5.2f} TB/s)",
          flush=True)
    return us


cl = torch.channels_last
B, T, FR = 32, 250, 64
x = (torch.randn(B, 4, T, FR, device=dev) * 20 - 30).to(torch.bfloat16).contiguous(memory_format=cl)
w = (torch.randn(64, 4, 3, 3, device=dev) * 0.1).to(torch.bfloat16).contiguous(memory_format=cl)
gamma, beta = torch.ones(64, device=dev), torch.zeros(64, device=dev)
rm, rv = torch.zeros(64, device=dev), torch.ones(64, device=dev)
go = torch.randn(B, 64, T, FR // 2, device=dev).to(torch.bfloat16).contiguous(memory_format=cl)
dw = torch.empty_like(w)
mb_in, mb_x1, mb_y = x.numel() * 2 / 1e6, B * 64 * T * FR * 2 / 1e6, go.numel() * 2 / 1e6

print(f"first block, B = {B}, T = {T}, F = {FR}: in {mb_in:.1f} MB, x1 / dx1 {mb_x1:.1f} MB, y / dy {mb_y:.1f} MB")
print("general path")
x1 = F.conv2d(x, w, padding=1)
t_old_f = line("library convolution (in -> x1)", timeit(lambda: F.conv2d(x, w, padding=1)), mb_in + mb_x1)
t_old_f += line("conv_tail_forward (stats, finalise, apply)",
                timeit(lambda: seld_native.conv_tail_forward(x1, gamma, beta, rm, rv, 0.1, 1e-5, True, 2)), 2 * mb_x1 + mb_y)
_, mean_invstd, scale_shift = seld_native.conv_tail_forward(x1, gamma, beta, rm, rv, 0.1, 1e-5, True, 2)
t_old_b = line("conv_tail_backward (reduce, finalise, apply)",
               timeit(lambda: seld_native.conv_tail_backward(x1, go, mean_invstd, scale_shift, 2)), 3 * mb_x1 + 2 * mb_y)
dx1 = seld_native.conv_tail_backward(x1, go, mean_invstd, scale_shift, 2)[0]


def library_wgrad():
    dw.copy_(torch.ops.aten.convolution_backward(dx1, x, w, None, (1, 1), (1, 1), (1, 1), False, (0, 0), 1,
                                                 (False, True, False))[1])


t_old_b += line("library weight gradient + copy (dx1, in -> dW)", timeit(library_wgrad), mb_x1 + mb_in)
print(f"  forward {t_old_f:.1f} us, backward {t_old_b:.1f} us")

print("first-block kernels (csrc/convfirst.hip)")
fwd = lambda phases: seld_native.convfirst_forward(x, w, gamma, beta, rm, rv, 0.1, 1e-5, phases=phases)
_, mean_invstd, scale_shift = fwd(3)
bwd = lambda phases: seld_native.convfirst_backward(x, w, go, mean_invstd, scale_shift, dw, phases=phases)
bwd(3)
line("statistics (in -> partials)", timeit(lambda: fwd(1)), mb_in)
line("finalise + apply (in -> y)", timeit(lambda: fwd(2)), mb_in + mb_y)
t_new_f = line("forward, both launches", timeit(lambda: fwd(3)), 2 * mb_in + mb_y)
line("backward reduce (in, dy -> partials)", timeit(lambda: bwd(1)), mb_in + mb_y)
line("finalise + weight gradient + sum (-> dW)", timeit(lambda: bwd(2)), mb_in + mb_y)
t_new_b = line("backward, all launches      ", timeit(lambda: bwd(3)), 2 * (mb_in + mb_y))
print(f"  forward {t_new_f:.1f} us ({t_old_f / t_new_f:.2f}x), backward {t_new_b:.1f} us ({t_old_b / t_new_b:.2f}x)")
