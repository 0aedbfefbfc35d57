"""Records tests/golden/conv3x3_loop_parent.npz, the fixture of tests/test_conv_loop_parent_bits_gpu.py: the bit patterns
that csrc/convfwd.hip (outputs and ``partials`` rows) and csrc/convdgrad.hip write for the test's seeded CPU inputs.

    SELD_HIP_LIB=<libseld_hip.so of the commit to record> python tools/record_conv_loop_fixture.py [OUT.npz]

The fixture holds the results of the commit BEFORE the loop's loads were rescheduled; it is recorded once from that
commit's build and not again from a later one (a later build has to reproduce it)."""
import sys
from pathlib import Path
ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "sound-event-localization-detection_amd"), str(ROOT / "tests")]
import numpy as np
import torch
import seld_native
import test_conv_loop_parent_bits_gpu as t

dev = torch.device("cuda:0")
out = Path(sys.argv[1]) if len(sys.argv) > 1 else t.FIXTURE
arrays = {}
for shape in t.FWD:
    plain, y, partials = t.run_forward(seld_native, shape, dev)
    assert torch.equal(plain, y)
    arrays[t.key("fwd", shape, "y")] = t.bits(y)
    arrays[t.key("fwd", shape, "partials")] = t.bits(partials)
for shape in t.DGRAD:
    arrays[t.key("dgrad", shape, "dx")] = t.bits(t.run_dgrad(seld_native, shape, dev))
np.savez_compressed(out, **arrays)
print(f"{seld_native.LIB_PATH}: {len(arrays)} arrays, {sum(a.nbytes for a in arrays.values())} bytes -> {out} "
      f"({out.stat().st_size} bytes)")
