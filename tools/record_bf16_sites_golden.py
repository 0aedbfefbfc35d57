"""Records tests/golden/bf16_sites_parent.npz: the bf16 bit patterns (uint16) that the kernels of the commit BEFORE
csrc/seld_bf16.h store for the cases of tests/bf16_sites_cases.py.  Run once, on a GPU, with SELD_HIP_LIB pointing at a
build of that commit's library; tests/test_bf16_sites_gpu.py compares every later build with it.

usage: SELD_HIP_LIB=/path/to/parent/libseld_hip.so python tools/record_bf16_sites_golden.py [output.npz]"""
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "sound-event-localization-detection_amd"), str(ROOT / "tests")]
import numpy as np
import torch
import seld_native
import bf16_sites_cases as cases


def main():
    out = Path(sys.argv[1]) if len(sys.argv) > 1 else ROOT / "tests" / "golden" / "bf16_sites_parent.npz"
    seld_native.load_library()
    arrays = {name: cases.bits(t) for name, t in cases.run(seld_native, torch.device("cuda:0")).items()}
    out.parent.mkdir(parents=True, exist_ok=True)
    np.savez_compressed(out, **arrays)
    print(f"{out}: {len(arrays)} arrays, {out.stat().st_size} bytes, library {seld_native.LIB_PATH}")


if __name__ == "__main__":
    main()
