"""Spatial-feature micro-benchmark (developer tool; target of rocprofv3 --kernel-trace --stats).
usage: python tools/bench_spatial.py [kind logmel_gcc|logmel_iv] [channels] [n_clips] [reps]
       python tools/bench_spatial.py logmel_nipd [channels] [n_clips] [reps] [out.json]
           the NIPD kernel (default range and full range) and the GCC-PHAT kernel on the SAME phasor words, alternating in one
           process; then both feature sets end to end and the window gather at their channel counts"""
import sys
from pathlib import Path
ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "sound-event-localization-detection_amd")]
import torch
import seld_native

kind = sys.argv[1] if len(sys.argv) > 1 else "logmel_gcc"
channels = int(sys.argv[2]) if len(sys.argv) > 2 else 8
n_clips = int(sys.argv[3]) if len(sys.argv) > 3 else 8
reps = int(sys.argv[4]) if len(sys.argv) > 4 else 5
dev = torch.device("cuda:0")
L = 1440000


def _median_ms(fns, reps):
    """Median time of each callable, the callables taking turns (one event pair per call)."""
    times = [[] for _ in fns]
    for _ in range(reps):
        for i, fn in enumerate(fns):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            times[i].append(e0.elapsed_time(e1))
    return [sorted(t)[len(t) // 2] for t in times]


def bench_nipd(channels, n_clips, reps, out_path):
    import ctypes
    import json
    lib = seld_native.load_library()
    x = torch.randn(n_clips, channels, L, device=dev) * 0.1
    frames, pitch = seld_native.num_frames(L), int(lib.seld_phasor_pitch())
    seld_native.ensure_init(dev)
    p, stream = seld_native._p, seld_native._stream_ptr(dev)
    logmel = torch.empty((n_clips, frames, channels, 64), device=dev)
    words = torch.empty((n_clips, channels, frames, pitch), dtype=torch.int32, device=dev)
    seld_native.check(lib.seld_logmel_phasors_f32(p(x), n_clips, channels, L, p(logmel), frames * channels * 64, 64, 1,
                                                   channels * 64, p(words), stream), "seld_logmel_phasors_f32")
    pairs = channels * (channels - 1) // 2
    gcc_out = torch.empty((n_clips, frames, pairs, 64), device=dev)
    nipd_out = torch.empty((n_clips, frames, channels - 1, 64), device=dev)
    ranges = {"default": (None, None), "full": (25.0, 12000.0)}
    tables = {k: seld_native.nipd_table(dev, lo, hi) for k, (lo, hi) in ranges.items()}

    def gcc():
        seld_native.check(lib.seld_gcc_phat_q15(p(words), n_clips, channels, frames, p(gcc_out), frames * pairs * 64, 64, 1,
                                                pairs * 64, stream), "seld_gcc_phat_q15")
    fns = [lambda: seld_native.nipd_q15(words, nipd_out, tables["default"][1]), gcc,
           lambda: seld_native.nipd_q15(words, nipd_out, tables["full"][1])]
    for fn in fns * 3:
        fn()
    torch.cuda.synchronize()
    t_default, t_gcc, t_full = _median_ms(fns, reps)
    rows = n_clips * frames

    def nipd_bytes(host):
        first, taps = host[0], host[1]
        live = taps > 0
        lo, hi = int(first[live].min()), int((first + taps)[live].max()) - 1
        return rows * (channels * 4 * (hi - lo + 1) + (channels - 1) * 256), hi - lo + 1
    b_default, bins_default = nipd_bytes(tables["default"][0])
    b_full, bins_full = nipd_bytes(tables["full"][0])
    b_gcc = rows * (channels * 4 * 481 + pairs * 256)
    result = {"clips": n_clips, "channels": channels, "seconds_per_clip": L / 24000, "frames": rows, "reps": reps,
              "nipd_default": {"ms": t_default, "bins": bins_default, "algorithmic_bytes": b_default,
                               "GB_per_s": b_default / t_default / 1e6},
              "nipd_full": {"ms": t_full, "bins": bins_full, "algorithmic_bytes": b_full, "GB_per_s": b_full / t_full / 1e6},
              "gcc_q15": {"ms": t_gcc, "bins": 481, "algorithmic_bytes": b_gcc, "GB_per_s": b_gcc / t_gcc / 1e6}}
    del gcc_out, nipd_out, words, logmel
    # both feature sets end to end from PCM
    ends = [lambda: seld_native.spatial_features(x, "logmel_nipd"), lambda: seld_native.spatial_features(x, "logmel_gcc")]
    for fn in ends * 2:
        fn()
    torch.cuda.synchronize()
    e_nipd, e_gcc = _median_ms(ends, max(3, reps // 4))
    result["features_end_to_end_ms"] = {"logmel_nipd": e_nipd, "logmel_gcc": e_gcc}
    # the window gather (32 windows of 250 frames) at the two sets' channel counts
    gathers = {}
    starts = torch.arange(0, 32 * 125, 125, dtype=torch.int64, device=dev)
    for total in (2 * channels - 1, channels + pairs):
        src = torch.randn(frames, total, 64, device=dev)
        fn = lambda: seld_native.gather_windows(src, starts, 250)
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        gathers[str(total)] = {"ms": _median_ms([fn], reps)[0], "bytes": 2 * 32 * 250 * total * 256}
    result["window_gather_32x250"] = gathers
    print(json.dumps(result))
    if out_path:
        Path(out_path).parent.mkdir(parents=True, exist_ok=True)
        Path(out_path).write_text(json.dumps(result, indent=1) + "\n")


if kind == "logmel_nipd":
    bench_nipd(channels, n_clips, reps if len(sys.argv) > 4 else 20, sys.argv[5] if len(sys.argv) > 5 else None)
    sys.exit(0)
x = torch.randn(n_clips, channels, L, device=dev) * 0.1
for _ in range(2):
    out = seld_native.spatial_features(x, kind)
torch.cuda.synchronize()
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
e0.record()
for _ in range(reps):
    out = seld_native.spatial_features(x, kind)
e1.record()
torch.cuda.synchronize()
ms = e0.elapsed_time(e1) / reps
byt = n_clips * (channels * L * 4 + out.shape[2] * 64 * out.shape[1] * 4)
print(f"{kind} {channels}ch clips={n_clips}: {ms:.3f} ms/call {byt / ms / 1e6:.1f} GB/s algorithmic ({byt / 1e6:.1f} MB/call), "
      f"frac {byt / ms / 1e6 / 8000:.4f}")
