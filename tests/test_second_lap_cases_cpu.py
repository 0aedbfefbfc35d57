"""CPU checks of tests/second_lap_cases.py, so that tests/test_second_lap_gpu.py cannot pass vacuously: with the library
limited to one compute unit every launch of every case walks at least three laps with a ragged last one (the caps are the
host's own conditions, restated in the table), and every line of csrc/ that reads ``num_cus`` is named by a case or by the
exemption list."""
import re
from pathlib import Path

import pytest

import second_lap_cases as table

CSRC = Path(__file__).resolve().parent.parent / "sound-event-localization-detection_amd" / "csrc"


def _hits():
    """(file name, source line without its comment) of every line of csrc/*.hip and *.h that reads num_cus in code"""
    out = []
    for path in sorted(list(CSRC.glob("*.hip")) + list(CSRC.glob("*.h"))):
        for line in path.read_text().splitlines():
            code = line.split("//")[0]
            if re.search(r"\bnum_cus\b", code):
                out.append((path.name, " ".join(code.split())))
    return out


@pytest.mark.parametrize("case", table.CASES, ids=[c.name for c in table.CASES])
def test_every_launch_walks_three_laps_and_a_ragged_last_one_on_one_cu(case):
    launches = case.launches(case.shape, 1)
    assert launches
    for launch in launches:
        label, items, per_group, grid = launch
        assert grid >= 1 and items > 0
        assert table.laps(launch) >= 3, (case.name, launch)
        assert table.ragged(launch), (case.name, launch)


def test_case_names_are_unique_and_every_case_has_a_runner_and_a_judge():
    names = [c.name for c in table.CASES]
    assert len(set(names)) == len(names)
    worker = (Path(__file__).resolve().parent / "second_lap_worker.py").read_text()
    for case in table.CASES:
        assert f"def run_{case.name}(" in worker, case.name
        assert case.judge and case.entry and case.sites


def test_every_line_that_reads_num_cus_is_named_by_a_case_or_exempt():
    named = {(f, " ".join(piece.split())) for c in table.CASES for f, piece in c.sites}
    exempt = {(f, " ".join(piece.split())) for f, piece in table.EXEMPT}
    assert not named & exempt
    hits = _hits()
    assert len(hits) >= 40                                         # the search itself found the launch sites
    missing = [(f, code) for f, code in hits
               if not any(f == nf and piece in code for nf, piece in named | exempt)]
    assert not missing, "launch sites sized from num_cus without a second-lap case:\n" + "\n".join(f"{f}: {c}" for f, c in missing)
    # and nothing in the table names a line that is gone
    stale = [(f, piece) for f, piece in named | exempt if not any(f == hf and piece in code for hf, code in hits)]
    assert not stale, stale
    assert all(reason for reason in table.EXEMPT.values())
