"""Records tests/golden/frontend_parent.npz: what the front-end kernels (csrc/logmel.hip, spatial.hip, nipd.hip) of the
commit BEFORE their shared wave pipeline and launch prologue write for the seeded clips of tests/frontend_parent_cases.py.
Run once, on a GPU, with that commit's library (SELD_HIP_LIB points at it); tests/test_frontend_parent_bits_gpu.py compares
every later build with it.  Results of at most 64 KB are kept as uint32 bit patterns, larger ones (the spectra, the phasor
words, the 28-channel GCC features) as shape, dtype and SHA-256.

usage: SELD_HIP_LIB=parent/libseld_hip.so python tools/record_frontend_parent_golden.py [output.npz]"""
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "sound-event-localization-detection_amd"), str(ROOT / "tests")]
import numpy as np
import torch
import seld_native
import frontend_parent_cases as cases


def main():
    out = Path(sys.argv[1]) if len(sys.argv) > 1 else ROOT / "tests" / "golden" / "frontend_parent.npz"
    dev = torch.device("cuda:0")
    arrays = {}
    for length in cases.LENGTHS:
        for dtype in cases.DTYPES:
            first = cases.run(seld_native, dev, length, dtype)
            again = cases.run(seld_native, dev, length, dtype)
            for name, x in first.items():
                if not torch.equal(x, again[name]):
                    raise SystemExit(f"{cases.key(length, dtype, name)}: two runs of this library differ")
                arrays[cases.key(length, dtype, name)] = cases.record(name, x)
    out.parent.mkdir(parents=True, exist_ok=True)
    np.savez_compressed(out, **arrays)
    print(f"{out}: {len(arrays)} arrays, {out.stat().st_size} bytes, library {seld_native.LIB_PATH}")


if __name__ == "__main__":
    main()
