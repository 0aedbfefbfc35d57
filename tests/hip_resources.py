"""The compiler's own resource report of a .hip file's kernels (hipcc -Rpass-analysis=kernel-resource-usage, gfx950), for
the CPU tests that hold kernels to "no scratch" and to their LDS budget.  Nothing is linked or run."""
import re
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
FIELDS = (("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"), ("lds", r"LDS Size \[bytes/block\]: (\d+)"),
          ("vgprs", r" VGPRs: (\d+)"), ("sgprs", r"TotalSGPRs: (\d+)"), ("occupancy", r"Occupancy \[waves/SIMD\]: (\d+)"))


def report(path) -> dict:
    """{mangled kernel name: {scratch, lds, vgprs, sgprs, occupancy}} of the kernels ``path`` compiles to."""
    run = subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", f"-I{ROOT / 'include'}",
                          "-Rpass-analysis=kernel-resource-usage", "-c", str(path), "-o", "/dev/null"],
                         capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-2000:]
    found, current = {}, None
    for line in run.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            current = found.setdefault(m.group(1), {})
        for key, pattern in FIELDS:
            m = re.search(pattern, line)
            if m and current is not None:
                current[key] = int(m.group(1))
    return found


if __name__ == "__main__":              # python tests/hip_resources.py a.hip b.hip: one line per kernel
    for arg in sys.argv[1:]:
        for kernel, row in report(arg).items():
            print(Path(arg).name, kernel, " ".join(f"{k}={v}" for k, v in row.items()))
