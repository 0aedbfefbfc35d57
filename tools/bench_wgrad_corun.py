"""Developer experiment: does the convolution weight-gradient kernel (csrc/convwgrad.hip) leave room on the chip for
the HBM-bound BatchNorm tail backward (csrc/convtail.hip) that runs beside it in the captured iteration?

conv_tail_backward at encoder block 2's shape (C = 128, rows = 32 * 250 * 32) on the current stream, conv3x3_wgrad at
block 4's shape (256 -> 512 channels, F = 8) on a second stream, both released by one event behind a long GEMM so that
every launch is queued before either starts.  HIP events: each alone, the tail's time per call while weight gradients
cover its whole run, and the weight gradient's time per call while tails cover its whole run.  7 alternating samples of
20 calls, median (min - max) in us per call.  usage: python tools/bench_wgrad_corun.py [label]"""
import statistics
import sys
from pathlib import Path
ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "sound-event-localization-detection_amd")]
import torch
import seld_native

SAMPLES, CALLS = 7, 20
label = sys.argv[1] if len(sys.argv) > 1 else "this build"
dev = torch.device("cuda:0")
cl = torch.channels_last

# tail: block 2 (pre-pool [32, 128, 250, 32], pool 2)
xt = torch.randn(32, 128, 250, 32, device=dev).to(torch.bfloat16).contiguous(memory_format=cl)
bn_w, bn_b = torch.rand(128, device=dev) + 0.5, torch.randn(128, device=dev)
yt, mi, ss = seld_native.conv_tail_forward(xt, bn_w, bn_b, torch.zeros(128, device=dev), torch.ones(128, device=dev),
                                           0.1, 1e-5, True, 2)
go = torch.randn_like(yt)
# weight gradient: block 4
xw = torch.randn(32, 256, 250, 8, device=dev).to(torch.bfloat16).contiguous(memory_format=cl)
dyw = torch.randn(32, 512, 250, 8, device=dev).to(torch.bfloat16).contiguous(memory_format=cl)
dw = torch.empty(512, 256, 3, 3, device=dev, dtype=torch.bfloat16).contiguous(memory_format=cl)
plug_a = torch.randn(8192, 8192, device=dev, dtype=torch.bfloat16)
plug_out = torch.empty_like(plug_a)

main = torch.cuda.current_stream(dev)
side = torch.cuda.Stream(dev)


def tail():
    seld_native.conv_tail_backward(xt, go, mi, ss, 2)


def wgrad():
    seld_native.conv3x3_wgrad(xw, dyw, dw)


def run(n_tail, n_wgrad):
    """n_tail tails on the main stream and n_wgrad weight gradients on the side stream from one event; us per call of
    each (None for a count of 0)."""
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    torch.mm(plug_a, plug_a, out=plug_out)                 # ~1 ms: the launches below are queued before it ends
    ev[0].record(main)
    side.wait_event(ev[0])
    with torch.cuda.stream(side):
        for _ in range(n_wgrad):
            wgrad()
        ev[2].record(side)
    for _ in range(n_tail):
        tail()
    ev[1].record(main)
    main.wait_event(ev[2])
    torch.cuda.synchronize()
    return (ev[0].elapsed_time(ev[1]) / n_tail * 1e3 if n_tail else None,
            ev[0].elapsed_time(ev[2]) / n_wgrad * 1e3 if n_wgrad else None)


for _ in range(3):
    run(CALLS, CALLS)
t_alone = statistics.median(run(CALLS, 0)[0] for _ in range(3))
w_alone = statistics.median(run(0, CALLS)[1] for _ in range(3))
cover_w = min(200, int(CALLS * t_alone / w_alone * 3) + 4)          # weight gradients that outlast 20 tails
cover_t = min(400, int(CALLS * w_alone / t_alone * 3) + 4)          # tails that outlast 20 weight gradients

cols = {"tail alone": [], "wgrad alone": [], "tail beside wgrad": [], "wgrad beside tail": []}
for _ in range(SAMPLES):
    cols["tail alone"].append(run(CALLS, 0)[0])
    cols["tail beside wgrad"].append(run(CALLS, cover_w)[0])
    cols["wgrad alone"].append(run(0, CALLS)[1])
    cols["wgrad beside tail"].append(run(cover_t, CALLS)[1])

print(f"{label}: {torch.cuda.get_device_name(0)}, {SAMPLES} alternating samples of {CALLS} calls, us per call, "
      f"median (min - max); cover: {cover_w} wgrad / {cover_t} tail calls")
for name, v in cols.items():
    print(f"  {name:18s} {statistics.median(v):7.1f} ({min(v):7.1f} - {max(v):7.1f})", flush=True)
