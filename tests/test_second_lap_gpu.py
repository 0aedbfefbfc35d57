"""Every CU-capped kernel on its second and later laps (tests/second_lap_cases.py): tests/second_lap_worker.py runs ONCE in
a fresh process with SELD_CUS=1, so that the library sizes its grids for one compute unit, and judges every case against the
reference of the kernel's own test module; the tests here assert one case each from the worker's lines.  Three more child
processes, which only initialise the library, check how seld_init reads SELD_CUS.

Worker wall time, measured on an MI355X machine: 3.2 s started from a shell, 4.3 - 4.7 s as this module's fixture (of which
1.1 s are the 25 cases, float64 references included; the rest is the import of torch and the library's initialisation).
MEASURED_SECONDS rounds that up to 5; the timeout is three times that."""
import json
import os
import subprocess
import sys
from pathlib import Path

import pytest

import second_lap_cases as table

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
WORKER = Path(__file__).resolve().parent / "second_lap_worker.py"
MEASURED_SECONDS = 5
TIMEOUT = 3 * MEASURED_SECONDS


@pytest.fixture(scope="module")
def worker(gpu_device):
    """name -> the worker's record; started once, never again.  A worker that was killed or left with a non-zero status
    fails every case with its output."""
    state = {"cases": {}, "failure": None}
    try:
        out = subprocess.run([sys.executable, str(WORKER)], env=dict(os.environ, SELD_CUS="1"), capture_output=True, text=True,
                             timeout=TIMEOUT, cwd=str(ROOT))
    except subprocess.TimeoutExpired as e:
        state["failure"] = f"the worker was killed after {TIMEOUT} s\n{str(e.stdout)[-3000:]}\n{str(e.stderr)[-3000:]}"
        return state
    for line in out.stdout.splitlines():
        if line.startswith("CASE "):
            record = json.loads(line[5:])
            state["cases"][record["name"]] = record
    if out.returncode != 0:
        state["failure"] = f"the worker exited with {out.returncode}\n{out.stdout[-3000:]}\n{out.stderr[-3000:]}"
    return state


@pytest.mark.parametrize("case", table.CASES, ids=[c.name for c in table.CASES])
def test_case_on_one_cu(worker, case):
    assert worker["failure"] is None, worker["failure"]
    record = worker["cases"].get(case.name)
    assert record is not None, f"the worker printed no line for {case.name}"
    print(record)
    assert record["differing"] == 0, record
    assert record["worst"] <= 1.0, record
    assert record["ok"], record


INIT = ("import ctypes, sys, torch; sys.path.insert(0, sys.argv[1]); import seld_native; lib = seld_native.load_library(); "
        "torch.cuda.set_device(0); rc = lib.seld_init(0); message = lib.seld_last_error().decode() if rc else ''; "
        "print('INIT', rc, lib.seld_num_cus(), torch.cuda.get_device_properties(0).multi_processor_count, message)")


def _init(value):
    out = subprocess.run([sys.executable, "-c", INIT, str(ROOT / "sound-event-localization-detection_amd")],
                         env=dict(os.environ, SELD_CUS=value), capture_output=True, text=True, timeout=120, cwd=str(ROOT))
    assert out.returncode == 0, out.stderr[-2000:]
    line = next(x for x in out.stdout.splitlines() if x.startswith("INIT "))
    _, rc, cus, device_cus, *message = line.split(" ", 4)
    return int(rc), int(cus), int(device_cus), " ".join(message)


@pytest.mark.parametrize("value", ["0", "abc"])
def test_init_refuses_a_limit_that_is_no_positive_integer(gpu_device, value):
    rc, cus, _, message = _init(value)
    assert rc == -1 and "SELD_CUS" in message                       # kErrInvalidArgument, naming the variable
    assert cus == -3                                                # nothing was initialised


def test_init_never_raises_the_count(gpu_device):
    rc, cus, device_cus, _ = _init("100000")
    assert rc == 0 and cus == device_cus and device_cus >= 1
