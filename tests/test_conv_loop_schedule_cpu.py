"""CPU check of what the compiler makes of the main loop of csrc/conv3x3_loop.h (hipcc -S for gfx950; nothing is
linked or run), for every instantiation of conv3x3_fwd_kernel (convfwd.hip) and conv3x3_dgrad_kernel (convdgrad.hip).

The loop's source says that the next stage's weight slice is in flight under this stage's MFMAs and that the position
fragments are read ahead of the MFMAs that use them.  The compiler is free to undo both (it once merged the loads of
the slice into the loop header and waited for them right behind the barrier, and it read every fragment just before
its MFMAs), so the two properties are read off the assembly:

  * weight loads: going round the loop in program order from a load of the slice, at least three quarters of the
    loop's MFMAs come before the ``s_waitcnt vmcnt`` that guards the ``ds_write`` of the loaded registers into the
    weight buffer (an LDS-DMA load has no ds_write: there the next ``s_waitcnt vmcnt`` is its guard);
  * fragment waits: at most a quarter of the MFMA groups (runs of MFMAs with no s_waitcnt between them) have an
    ``s_waitcnt`` with ``lgkmcnt(0)`` between them and the previous MFMA.

AFTER EVERY ROCm / compiler update run this file, like tests/test_conv_wgrad_occupancy_cpu.py."""
import functools
import re
import subprocess
from pathlib import Path

import pytest

CSRC = Path(__file__).resolve().parent.parent / "sound-event-localization-detection_amd" / "csrc"
KERNELS = {"convfwd.hip": ("conv3x3_fwd_kernel", 12), "convdgrad.hip": ("conv3x3_dgrad_kernel", 6)}


@functools.lru_cache(maxsize=None)
def _assembly(source):
    run = subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950",
                          f"-I{CSRC.parent.parent / 'include'}", "--cuda-device-only", "-S", str(CSRC / source),
                          "-o", "-"], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-2000:]
    return run.stdout


def _kernels(text, name):
    """{mangled name: instruction and label lines} of the kernels whose name holds ``name``."""
    found, current = {}, None
    for line in text.splitlines():
        m = re.match(r"(_Z\w+):", line)
        if m:
            current = found.setdefault(m.group(1), []) if name in m.group(1) else None
            continue
        if current is None:
            continue
        s = line.strip()
        if s.startswith("s_endpgm"):
            current = None
        elif s and not s.startswith(".") or s.startswith(".LBB"):
            current.append(s)
    return found


def _main_loop(lines):
    """The innermost loop that holds the MFMAs, as the instructions of one trip round it in execution order from the
    loop header: the trip through the fewest basic blocks, i.e. a stage that stages no image (whose blocks the
    compiler lays out wherever it likes, some of them behind the loop's last branch)."""
    blocks = []                                 # [label, header of the loop it belongs to or None, instructions]
    for s in lines:
        if s.startswith(".LBB") or s.startswith("; %bb."):
            label = s.split(":")[0]
            m = re.search(r"Header=(BB\d+_\d+)", s)
            blocks.append([label, m.group(1) if m else (label[2:] if "Loop Header" in s else None), []])
        elif blocks and not s.startswith(";"):
            blocks[-1][2].append(s)
    mfma = [k for k, b in enumerate(blocks) if any(i.startswith("v_mfma") for i in b[2])]
    assert len(mfma) == 1 and blocks[mfma[0]][1] is not None, "the MFMAs are one basic block inside a loop"
    header = blocks[mfma[0]][1]
    index = {b[0]: k for k, b in enumerate(blocks)}

    def successors(k):
        ins = blocks[k][2]
        out = [index[i.split()[1]] for i in ins if i.startswith(("s_cbranch", "s_branch"))]
        if not (ins and ins[-1].startswith("s_branch")) and k + 1 < len(blocks):
            out.append(k + 1)
        return [j for j in out if blocks[j][1] == header]

    def path(src, dst):
        seen, frontier = {src: None}, [src]
        while frontier:
            nxt = []
            for k in frontier:
                for j in successors(k):
                    if j == dst:
                        out = [k]
                        while seen[out[-1]] is not None:
                            out.append(seen[out[-1]])
                        return out[::-1]
                    if j not in seen:
                        seen[j] = k
                        nxt.append(j)
            frontier = nxt
        raise AssertionError("no path round the loop")

    head = index[".L" + header]
    trip = path(head, mfma[0]) + path(mfma[0], head) if head != mfma[0] else path(head, head)
    return [i for k in trip for i in blocks[k][2]]


def _regs(operand):
    m = re.match(r"v\[(\d+):(\d+)\]", operand)
    if m:
        return set(range(int(m.group(1)), int(m.group(2)) + 1))
    m = re.match(r"v(\d+)$", operand)
    return {int(m.group(1))} if m else set()


def _image_bytes(kernel):
    f = int(re.search(r"kernelILi(\d+)E", kernel).group(1))
    return (256 // f + 2) * (f + 2) * 160


def _weight_load_cover(kernel, loop):
    """For every load of the weight slice: the share of the loop's MFMAs between it and its guard."""
    n, total = len(loop), sum(i.startswith("v_mfma") for i in loop)
    covers = []
    for k, ins in enumerate(loop):
        if not (ins.startswith("global_load") or ins.startswith("buffer_load")):
            continue
        ring = [loop[(k + 1 + j) % n] for j in range(n - 1)]
        if " lds" in ins or "_lds_" in ins:
            guard = next(j for j, i in enumerate(ring) if i.startswith("s_waitcnt") and "vmcnt" in i)
        else:
            dest = _regs(ins.split()[1].rstrip(","))
            store = None
            for j, i in enumerate(ring):
                ops = [o.rstrip(",") for o in i.split()[1:]]
                if i.startswith("ds_write") and any(_regs(o) & dest for o in ops[1:]):
                    store = j
                    break
                if not i.startswith("ds_write") and ops and _regs(ops[0]) & dest and not i.startswith("s_"):
                    break                                   # the registers are written again: not staged through LDS
            if store is None:
                continue
            m = re.search(r"offset:(\d+)", ring[store])
            if not m or int(m.group(1)) < _image_bytes(kernel):
                continue                                    # a piece of the image, not of the weight slice
            guard = max(j for j, i in enumerate(ring[:store]) if i.startswith("s_waitcnt") and "vmcnt" in i)
        covers.append(sum(i.startswith("v_mfma") for i in ring[:guard]) / total)
    return covers


def _fragment_waits(loop):
    """(MFMA groups that follow an s_waitcnt lgkmcnt(0), MFMA groups)."""
    groups = waits = 0
    wait_seen, zero_seen = True, False          # since the previous MFMA
    for ins in loop:
        if ins.startswith("v_mfma"):
            groups += wait_seen
            waits += zero_seen
            wait_seen = zero_seen = False
        elif ins.startswith("s_waitcnt"):
            wait_seen = True
            zero_seen = zero_seen or "lgkmcnt(0)" in ins
    return waits, groups


@pytest.mark.parametrize("source", sorted(KERNELS))
def test_weight_prefetch_and_fragment_read_ahead_survive_the_compiler(source):
    name, count = KERNELS[source]
    kernels = _kernels(_assembly(source), name)
    assert len(kernels) == count, sorted(kernels)
    for kernel, lines in kernels.items():
        loop = _main_loop(lines)
        nt = int(re.search(r"kernelILi\d+ELi(\d+)E", kernel).group(1))
        covers = _weight_load_cover(kernel, loop)
        waits, groups = _fragment_waits(loop)
        print(kernel, "weight loads' MFMA cover", [round(c, 2) for c in covers], "lgkmcnt(0) groups", waits, "of", groups)
        assert len(covers) == nt // 32, (kernel, covers)               # 16-byte pieces per thread and stage
        assert min(covers) >= 0.75, (kernel, covers)
        assert groups >= 2 and 4 * waits <= groups, (kernel, waits, groups)
