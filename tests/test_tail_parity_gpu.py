"""Exact float64 replay of the fused BatchNorm tails (csrc/convtail.hip) on the card: every width the kernels accept,
every mode, both dtypes, training and eval, the unrolled main loops, one- and two-row inputs, guard regions.

The kernels return the coefficients they used, so the element-wise stage is replayed exactly on the CPU
(oracle/convtail.py): the forward of modes 1 / 2 / 3 is compared bit for bit on every element, the gradients against
the replayed routing with derived per-element bounds (tests/tail_checks.py, which states every bound and its reason).
Each test prints the worst error / bound ratio of every check.
"""
import pytest
import torch

import tail_checks as tc

pytestmark = pytest.mark.gpu

WIDTHS = [8, 16, 32, 64, 128, 256, 512, 1024, 2048]
DTYPES = [torch.bfloat16, torch.float32]


def _dev(m, mode, device):
    """[rows, C] -> the channels-last [1, C, rows / w, w] activation the wrappers take (w = 2 for the pool)."""
    if m is None:
        return None
    rows, c = m.shape
    w = 2 if mode == 2 else 1
    return m.to(device).view(1, rows // w, w, c).permute(0, 3, 1, 2)


def _host(t):
    return None if t is None else t.permute(0, 2, 3, 1).reshape(-1, t.shape[1]).cpu()


def _run(case, mode, device, training=True, backward=True):
    """One forward (and backward) through seld_native -> the kernels' outputs as CPU tensors."""
    import seld_native
    pool = 1 if mode == 3 else mode
    x, res = _dev(case["x"], mode, device), _dev(case["res"], 1, device)
    rm, rv = case["rm0"].to(device), case["rv0"].to(device)
    y, mi, ss = seld_native.conv_tail_forward(x, case["weight"].to(device), case["bias"].to(device), rm, rv,
                                              case["momentum"], case["eps"], training, pool, residual=res)
    out = dict(y=_host(y), mean_invstd=mi.cpu(), scale_shift=ss.cpu(), running_mean=rm.cpu(), running_var=rv.cpu())
    if backward:
        got = seld_native.conv_tail_backward(x, _dev(case["dy"], 1, device), mi, ss, pool, residual=res)
        out.update(dx=_host(got[0]), dweight=got[1].cpu(), dbias=got[2].cpu(), dres=_host(got[3]) if mode == 3 else None)
    torch.cuda.synchronize()
    return out


def _report(what, ratios):
    print(f"\n{what}: {tc.fmt(ratios)}")
    assert tc.passes(ratios), tc.fmt(ratios)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
@pytest.mark.parametrize("mode", [1, 2, 3, 4])
@pytest.mark.parametrize("c", WIDTHS)
def test_every_width_every_mode(gpu_device, c, mode, dtype):
    """rows = 74: even for the pool, blocks with one row and blocks with none at the wide end."""
    case = tc.make_case(mode, dtype, rows=74, c=c, integer=False, seed=c)
    _report(f"C={c} mode={mode}", tc.run_checks(case, _run(case, mode, gpu_device), mode, exact_stats=False))


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
@pytest.mark.parametrize("rows", [74, 4098])
@pytest.mark.parametrize("c", WIDTHS)
def test_integer_inputs_give_exact_statistics(gpu_device, c, rows, dtype):
    """Integer inputs: every fp32 partial sum is exact in any order, so the mean is exact, the rest within one ulp.
    The statistics are what this case is for: at rows = 4098 it checks them and the forward only, and leaves the
    backward to rows = 74, to spare the CPU reference of up to 8.4 M elements per case."""
    case = tc.make_case(1, dtype, rows=rows, c=c, integer=True, seed=c + rows)
    small = rows == 74
    out = _run(case, 1, gpu_device, backward=small)
    _report(f"C={c} rows={rows}", tc.run_checks(case, out, 1, exact_stats=True, backward=small))


# (mode, C, dtype): the two-rows-in-flight loops of the apply kernels only run once the grid is capped at 8 blocks per CU
MAIN_LOOP = [(2, 64, torch.bfloat16), (1, 1024, torch.bfloat16), (3, 2048, torch.bfloat16), (4, 512, torch.bfloat16),
             (1, 1024, torch.float32), (4, 512, torch.float32)]


@pytest.mark.parametrize("mode,c,dtype", MAIN_LOOP, ids=[f"mode{m}-C{c}-{str(d)[6:]}" for m, c, d in MAIN_LOOP])
def test_unrolled_main_loops_are_reached(gpu_device, mode, c, dtype):
    """out_rows = 2 G P + P + 1 (G = 8 blocks per CU, P = rows per block): every slot runs the two-in-flight loop once,
    the first P + 1 slots the remainder loop once more, the rest nothing -- the smallest shape that does all three."""
    g = 8 * torch.cuda.get_device_properties(gpu_device).multi_processor_count
    p = 2048 // c
    out_rows = 2 * g * p + p + 1
    if mode == 2:
        out_rows += out_rows % 2
    rows = 2 * out_rows if mode == 2 else out_rows
    case = tc.make_case(mode, dtype, rows=rows, c=c, integer=False, seed=5)
    _report(f"mode={mode} C={c} rows={rows}", tc.run_checks(case, _run(case, mode, gpu_device), mode, exact_stats=False))


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
@pytest.mark.parametrize("mode", [1, 2, 3, 4])
@pytest.mark.parametrize("c", [128, 1024])
def test_eval_mode_replays_from_the_running_statistics(gpu_device, c, mode, dtype):
    case = tc.make_case(mode, dtype, rows=74, c=c, integer=False, seed=c + 1)
    out = _run(case, mode, gpu_device, training=False, backward=False)
    _report(f"eval C={c} mode={mode}", tc.run_checks(case, out, mode, exact_stats=True, training=False, backward=False))
    assert torch.equal(out["running_mean"], case["rm0"]) and torch.equal(out["running_var"], case["rv0"])


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
@pytest.mark.parametrize("mode", [1, 4])
@pytest.mark.parametrize("rows", [1, 2])
def test_one_and_two_rows(gpu_device, rows, mode, dtype):
    """rows = 1: variance 0, invstd = 1 / sqrt(eps), running_var blended with 0 (no n / (n - 1) at one row)."""
    case = tc.make_case(mode, dtype, rows=rows, c=64, integer=True, seed=rows)
    out = _run(case, mode, gpu_device)
    _report(f"rows={rows} mode={mode}", tc.run_checks(case, out, mode, exact_stats=True))
    if rows == 1:
        assert torch.equal(out["mean_invstd"][0], case["x"][0].float())
        want = tc.c_float(1.0 / (tc.c_float(1e-5) ** 0.5))
        assert (out["mean_invstd"][1] - want).abs().max().item() <= tc.ulp32(torch.tensor(want)).item()
        assert out["dweight"].abs().max().item() == 0.0


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
def test_large_mean_under_the_statistics_check(gpu_device, dtype):
    """mean >> std, the (4, 64, 50, 16) pool-2 case of tests/test_convtail_gpu.py with offset 3000: the shifted
    accumulation keeps the variance within the accumulation bound of the shifted data."""
    case = tc.make_case(2, dtype, rows=4 * 50 * 16, c=64, integer=False, seed=5, offset=3000.0)
    _report("offset 3000", tc.run_checks(case, _run(case, 2, gpu_device), 2, exact_stats=False))


def _sentinel(n, guard, dtype, device):
    """n elements of ``dtype`` inside a sentinel-filled buffer with ``guard`` elements on each side -> (buffer, pattern
    copy, the inner slice as a tensor of dtype)."""
    assert dtype == torch.bfloat16
    pattern = (torch.arange(n + 2 * guard, dtype=torch.int32) % 251 + 0x3F00).to(torch.int16).to(device)
    buf = pattern.clone()
    return buf, pattern, buf[guard:guard + n].view(torch.bfloat16)


@pytest.mark.parametrize("mode", [1, 2, 3, 4])
@pytest.mark.parametrize("c", [64, 1024])
def test_writes_nothing_outside_y_dx_dres(gpu_device, c, mode):
    """y, dx and dres are slices of sentinel-filled buffers with 64 C guard elements on each side, passed to the C ABI
    by address: the guards come back bit-identical and the slices hold what the wrappers return."""
    import seld_native
    rows, dtype = 74, torch.bfloat16
    case = tc.make_case(mode, dtype, rows=rows, c=c, integer=False, seed=c + 7)
    want = _run(case, mode, gpu_device)
    seld_native.ensure_init(gpu_device)
    lib = seld_native.load_library()
    pool = 1 if mode == 3 else mode
    out_rows = rows // 2 if mode == 2 else rows
    dev = lambda t: None if t is None else t.to(gpu_device).contiguous()
    x, res, dy = dev(case["x"]), dev(case["res"]), dev(case["dy"])
    w, b, rm, rv = dev(case["weight"]), dev(case["bias"]), dev(case["rm0"]), dev(case["rv0"])
    ptr = lambda t: None if t is None else t.data_ptr()
    guard = 64 * c
    ybuf, ypat, y = _sentinel(out_rows * c, guard, dtype, gpu_device)
    dxbuf, dxpat, dx = _sentinel(rows * c, guard, dtype, gpu_device)
    drbuf, drpat, dres = _sentinel(rows * c, guard, dtype, gpu_device)
    stats = torch.empty(2, 2, c, dtype=torch.float32, device=gpu_device)
    dwb = torch.empty(2, c, dtype=torch.float32, device=gpu_device)
    ws = torch.empty(lib.seld_conv_tail_workspace_floats(c), dtype=torch.float32, device=gpu_device)
    torch.cuda.synchronize()
    rc = lib.seld_conv_tail_forward(ptr(x), ptr(res), 1, rows, c, pool, ptr(w), ptr(b), ptr(rm), ptr(rv), 0.1, 1e-5, 1,
                                    ptr(y), ptr(stats[0]), ptr(stats[1]), ptr(ws), None)
    assert rc == 0, rc
    rc = lib.seld_conv_tail_backward(ptr(x), ptr(res), ptr(dy), 1, rows, c, pool, ptr(stats[0]), ptr(stats[1]), ptr(dx),
                                     ptr(dres) if mode == 3 else None, ptr(dwb[0]), ptr(dwb[1]), ptr(ws), None)
    assert rc == 0, rc
    torch.cuda.synchronize()
    for buf, pat, n in ((ybuf, ypat, out_rows * c), (dxbuf, dxpat, rows * c), (drbuf, drpat, rows * c)):
        assert torch.equal(buf[:guard], pat[:guard]) and torch.equal(buf[guard + n:], pat[guard + n:])
    if mode != 3:
        assert torch.equal(drbuf, drpat)                                       # no residual: dres is never touched
    bits = lambda t: t.contiguous().view(torch.int16)
    assert torch.equal(bits(y.view(out_rows, c).cpu()), bits(want["y"]))
    assert torch.equal(bits(dx.view(rows, c).cpu()), bits(want["dx"]))
    if mode == 3:
        assert torch.equal(bits(dres.view(rows, c).cpu()), bits(want["dres"]))
    assert torch.equal(dwb[0].cpu(), want["dweight"]) and torch.equal(dwb[1].cpu(), want["dbias"])


@pytest.mark.parametrize("mode", [1, 2, 3, 4])
def test_two_calls_are_bit_identical(gpu_device, mode):
    case = tc.make_case(mode, torch.bfloat16, rows=2050, c=256, integer=False, seed=9)
    a, b = _run(case, mode, gpu_device), _run(case, mode, gpu_device)
    for k, v in a.items():
        if v is not None:
            assert torch.equal(v.view(torch.int16) if v.dtype == torch.bfloat16 else v,
                               b[k].view(torch.int16) if v.dtype == torch.bfloat16 else b[k]), k
