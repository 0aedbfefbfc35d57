"""CPU checks of the first-block kernels (csrc/convfirst.hip): every kernel compiles for gfx950 without scratch (the
compiler's own resource report) and the coverage rule the host path relies on."""
import re
import subprocess
from pathlib import Path

CSRC = Path(__file__).resolve().parent.parent / "sound-event-localization-detection_amd" / "csrc"

KERNELS = ("convfirst_stats_kernel", "convfirst_stats_final_kernel", "convfirst_apply_kernel",
           "convfirst_bwd_reduce_kernel", "convfirst_bwd_final_kernel", "convfirst_wgrad_kernel",
           "convfirst_wgrad_sum_kernel")


def test_convfirst_kernels_do_not_spill():
    run = subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950",
                          f"-I{CSRC.parent.parent / 'include'}", "-Rpass-analysis=kernel-resource-usage", "-c",
                          str(CSRC / "convfirst.hip"), "-o", "/dev/null"], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-2000:]
    found, current = {}, None
    for line in run.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            current = m.group(1)
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
        if m and current:
            found[current] = int(m.group(1))
    for kernel in KERNELS:
        hits = {k: v for k, v in found.items() if kernel in k}
        assert len(hits) == 1, (kernel, sorted(found))
    assert len(found) == len(KERNELS), sorted(found)
    assert all(v == 0 for v in found.values()), found


def test_convfirst_coverage():
    """The encoder's first block (4 -> 64 channels, F = 64) and the other power-of-two frequency counts are covered;
    other channel counts (the 7-channel intensity set, the 36-channel MIC set, blocks 2-4) and frequency counts are not."""
    import ctypes
    lib_path = CSRC.parent / "libseld_hip.so"
    if not lib_path.exists():
        import __graft_entry__
        __graft_entry__.build()
    lib = ctypes.CDLL(str(lib_path))
    lib.seld_convfirst_supported.argtypes = [ctypes.c_int64] * 3
    for f in (16, 32, 64, 128, 256):
        assert lib.seld_convfirst_supported(f, 4, 64) == 1, f
    for f, cin, cout in ((64, 7, 64), (64, 36, 64), (64, 4, 128), (32, 64, 128), (48, 4, 64), (8, 4, 64), (512, 4, 64)):
        assert lib.seld_convfirst_supported(f, cin, cout) == 0, (f, cin, cout)
    lib.seld_convfirst_workspace_floats.restype = ctypes.c_int64
    lib.seld_convfirst_workspace_floats.argtypes = [ctypes.c_int]
    assert 0 < lib.seld_convfirst_workspace_floats(0) < lib.seld_convfirst_workspace_floats(1)
