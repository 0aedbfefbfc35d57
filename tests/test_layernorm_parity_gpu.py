"""Exact float64 replay of the fused LayerNorm [-> ReLU] (csrc/layernorm.hip) on the card: all 16 forward and all 16
backward instantiations (dtype x D x relu), row counts chosen by the kernels' states, input families that sit on the
edges (constant and near-constant rows, |mean| >> std, pre-activations on the ReLU edge, overflow, subnormals), guard
regions around every buffer, repeatability, the autograd wrapper and the Conformer's conv module.

y, mean, dweight and dbias are compared bit for bit with the replay (oracle/layernorm.py); rstd and dx against derived
bounds (tests/layernorm_checks.py, which states every bound and its reason).  Every test prints its error / bound
ratios; the last test prints the worst of each over the whole module, and the worst rsqrtf distance.
"""
import itertools

import pytest
import torch
import torch.nn as nn

import layernorm_checks as lc

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
DTYPES = [F32, BF16]
WIDTHS = [256, 512, 1024, 2048]
NAME = {F32: "fp32", BF16: "bf16"}

# rows -> the state reached: 1, 3, 4, 5 idle wavefronts in the LDS fold, one and two blocks; 61, 65 = 16 and 17 partial
# rows, the final kernel's group boundary; 2045 = 512 blocks, the last with one live wavefront; 2049 = the first row
# count at which a wavefront walks two rows
ROWS_EVERYWHERE = [5, 65, 2049]
ROWS_EDGES = [1, 3, 4, 61, 2045]

INSTANTIATIONS = list(itertools.product(DTYPES, WIDTHS, [False, True]))
EVERY = [(t, d, relu, rows) for (t, d, relu) in INSTANTIATIONS for rows in ROWS_EVERYWHERE]
EDGES = [(t, d, relu, rows) for (t, d, relu) in INSTANTIATIONS if d in (256, 2048) for rows in ROWS_EDGES]

WORST = {}
RSQRT = [0.0]


def _id(p):
    return f"{NAME[p[0]]}-D{p[1]}-relu{int(p[2])}-rows{p[3]}"


def _run(case, relu, device):
    """One forward and backward through seld_native -> the kernels' outputs as CPU tensors."""
    import seld_native
    x, dy, w, b = (case[k].to(device) for k in ("x", "dy", "weight", "bias"))
    y, stats = seld_native.layernorm_forward(x, w, b, case["eps"], relu)
    dx, dweight, dbias = seld_native.layernorm_backward(x, dy, w, b, stats, relu)
    torch.cuda.synchronize()
    assert y.dtype == x.dtype and dx.dtype == x.dtype
    return dict(y=y.cpu(), stats=stats.cpu(), dx=dx.cpu(), dweight=dweight.cpu(), dbias=dbias.cpu())


def _report(what, case, out, relu, rows_per_launch=None):
    ratios = lc.run_checks(case, out, relu, rows_per_launch)
    if lc.finite(out["stats"]):
        dist = lc.rsqrt_distance(case["x"], case["eps"], out["stats"])
        RSQRT[0] = max(RSQRT[0], dist)
        ratios["rsqrt ulps"] = dist
    print(f"\n{what}: {lc.fmt(ratios)}")
    ratios.pop("rsqrt ulps", None)
    for k, v in ratios.items():
        WORST[k] = max(WORST.get(k, 0.0), v if v == v else float("inf"))
    assert lc.passes(ratios), lc.fmt(ratios)
    for k in ("stats.mean", "forward.y", "mask.mask", "backward.dweight", "backward.dbias"):
        assert ratios[k] == 0.0, (k, ratios[k])                            # bit-equal to the replay
    return ratios


def test_the_parametrisation_launches_all_32_instantiations():
    """Every (dtype, D, relu) of the dispatch is in the list below, and every case of it runs forward AND backward
    (``_run``): 16 + 16 instantiations."""
    assert len(set(INSTANTIATIONS)) == 16
    assert {p[:3] for p in EVERY} == set(INSTANTIATIONS)
    for rows in ROWS_EVERYWHERE:
        assert {p[:3] for p in EVERY if p[3] == rows} == set(INSTANTIATIONS)
    assert {(p[0], p[2], p[3]) for p in EDGES if p[1] == 256} == set(itertools.product(DTYPES, [False, True], ROWS_EDGES))
    assert {(p[0], p[2], p[3]) for p in EDGES if p[1] == 2048} == set(itertools.product(DTYPES, [False, True], ROWS_EDGES))


@pytest.mark.parametrize("p", EVERY, ids=_id)
def test_every_instantiation(gpu_device, p):
    dtype, d, relu, rows = p
    case = lc.make_case("gaussian", dtype, rows, d)
    _report(_id(p), case, _run(case, relu, gpu_device), relu)


@pytest.mark.parametrize("p", EDGES, ids=_id)
def test_row_counts_at_the_kernels_state_changes(gpu_device, p):
    dtype, d, relu, rows = p
    case = lc.make_case("gaussian", dtype, rows, d, seed=1)
    _report(_id(p), case, _run(case, relu, gpu_device), relu)


@pytest.mark.parametrize("eps", [1e-3, 1e-12])
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("rows,d", [(65, 256), (5, 1024)])
def test_eps_crosses_the_abi_as_the_float_it_is(gpu_device, rows, d, dtype, eps):
    """The near-constant rows make eps decide rstd: a dropped, truncated or double-typed eps moves it by far more than
    the allowance."""
    for family in ("gaussian", "near_constant"):
        case = lc.make_case(family, dtype, rows, d, eps=eps)
        _report(f"{family} eps={eps}", case, _run(case, True, gpu_device), True)


FAMILY_SHAPES = [(65, 256), (5, 1024), (2049, 512)]


@pytest.mark.parametrize("relu", [False, True], ids=["plain", "relu"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("rows,d", FAMILY_SHAPES)
@pytest.mark.parametrize("family", ["constant", "near_constant", "offset", "near_zero"])
def test_input_families(gpu_device, family, rows, d, dtype, relu):
    case = lc.make_case(family, dtype, rows, d)
    out = _run(case, relu, gpu_device)
    _report(f"{family} {NAME[dtype]} {rows}x{d} relu={relu}", case, out, relu)
    if family == "constant":
        # x - mean is exactly 0: y is bias (relu(bias)) bit for bit, dweight exactly 0, rstd = 1 / sqrt(eps)
        b = case["bias"].double()
        want = (torch.where(b > 0, b, torch.zeros((), dtype=torch.float64)) if relu else b).expand(rows, d)
        want = lc.ol.round_bf16(want) if dtype == BF16 else want
        assert lc.mismatch(out["y"], want) == 0.0
        assert torch.equal(out["stats"][:, 0], case["x"][:, 0].float())
        assert out["dweight"].abs().max().item() == 0.0
        ref = torch.full((rows,), lc.ol.c_float(1e-5), dtype=torch.float64) ** -0.5
        assert lc.ratio((out["stats"][:, 1].double() - ref).abs(), lc.RSQRT_ULPS * lc.ulp32(ref)) <= 1.0
    if family == "near_zero":
        y = out["y"].double()
        zero = y == 0
        assert bool(zero.any()) and bool((y > 0).any())
        if not relu:                                   # the signed zeros the family promises reach the output
            assert bool((zero & torch.signbit(y)).any()) and bool((zero & ~torch.signbit(y)).any())


@pytest.mark.parametrize("relu", [False, True], ids=["plain", "relu"])
@pytest.mark.parametrize("d", [256, 2048])
def test_an_overflowing_row_stays_in_its_row(gpu_device, d, relu):
    """fp32, the last row holds 3e38 throughout: its sum overflows, mean = inf, xhat = NaN.  Nothing non-finite may
    reach another row; dweight takes a NaN in every column (fmaf(g, NaN, dw)), dbias only adds g and stays finite.
    The other rows are checked in full, with the grid the kernel really ran (``rows_per_launch`` of all 9 rows)."""
    rows = 9
    case = lc.make_case("gaussian", F32, rows, d, seed=2)
    case["x"][rows - 1] = 3e38
    out = _run(case, relu, gpu_device)
    assert not bool(torch.isfinite(out["stats"][rows - 1]).all())
    assert not bool(torch.isfinite(out["dx"][rows - 1]).any())
    for k in ("y", "stats", "dx"):
        assert bool(torch.isfinite(out[k][:rows - 1]).all()), k
    assert not bool(torch.isfinite(out["dweight"]).any())
    assert bool(torch.isfinite(out["dbias"]).all())
    rest = dict(case, x=case["x"][:rows - 1], dy=case["dy"][:rows - 1])
    got = dict(out, y=out["y"][:rows - 1], stats=out["stats"][:rows - 1], dx=out["dx"][:rows - 1],
               dweight=torch.zeros(d), dbias=out["dbias"])
    ratios = lc.run_checks(rest, got, relu, rows_per_launch=4 * lc.ol.backward_blocks(rows))
    keep = [k for k in ratios if k.startswith(("stats.", "forward.", "mask."))] + ["backward.dx"]
    if relu:                                           # the overflowed row is masked out: it adds +0 to every column
        keep += ["backward.dbias", "backward.dbias_free"]
    ratios = {k: ratios[k] for k in keep}
    print("\n" + lc.fmt(ratios))
    assert lc.passes(ratios), lc.fmt(ratios)


@pytest.mark.parametrize("relu", [False, True], ids=["plain", "relu"])
@pytest.mark.parametrize("d", [256, 1024])
def test_subnormal_row_zero_weights_zero_gradient(gpu_device, d, relu):
    """bf16: one row of subnormal values (k * 2^-133), every third weight 0; then the same with dy = 0."""
    rows = 7
    case = lc.make_case("gaussian", BF16, rows, d, seed=3)
    k = torch.randint(-100, 101, (d,), generator=torch.Generator().manual_seed(d)).float()
    case["x"][3] = (k * 2.0 ** -133).bfloat16()
    assert bool((case["x"][3].float().abs() < 2.0 ** -126).all()) and bool((case["x"][3] != 0).any())
    case["weight"][::3] = 0.0
    _report("subnormal row, w = 0 columns", case, _run(case, relu, gpu_device), relu)
    case["dy"] = torch.zeros_like(case["dy"])
    out = _run(case, relu, gpu_device)
    _report("dy = 0", case, out, relu)
    for key in ("dx", "dweight", "dbias"):
        assert out[key].float().abs().max().item() == 0.0, key


# ------------------------------------------------------------------------------------------------- sentinels

_NAN = {BF16: 0x7FC0, F32: 0x7FC00000}
_BASE = {BF16: 0x3F00, F32: 0x3F000000}
_BITS = {BF16: torch.int16, F32: torch.int32}
GUARD = 4096                                                # elements; keeps every slice 16-byte aligned


def _guarded(n, dtype, device, nan=False):
    """n elements of ``dtype`` inside a buffer with GUARD sentinel (or NaN) elements on each side
    -> (buffer as integers, its untouched copy, the inner slice as ``dtype``)."""
    total = n + 2 * GUARD
    if nan:
        pattern = torch.full((total,), _NAN[dtype], dtype=torch.int32)
    else:
        pattern = torch.arange(total, dtype=torch.int32) % 251 + _BASE[dtype]
    pattern = pattern.to(_BITS[dtype]).to(device)
    buf = pattern.clone()
    return buf, pattern, buf[GUARD:GUARD + n].view(dtype)


def _guards_intact(buf, pattern, n):
    return torch.equal(buf[:GUARD], pattern[:GUARD]) and torch.equal(buf[GUARD + n:], pattern[GUARD + n:])


def _bits(t):
    return t.contiguous().view(_BITS[t.dtype])


@pytest.mark.parametrize("relu", [False, True], ids=["plain", "relu"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("rows,d", [(5, 256), (2049, 512)])
def test_nothing_is_read_or_written_outside_the_buffers(gpu_device, rows, d, dtype, relu):
    """Through the C ABI.  x and dy sit between NaN guards (an over-read poisons a result), y, dx, the statistics,
    dweight and dbias between sentinel guards (they come back bit-identical), the workspace is NaN-filled and twice
    the reported size (no partial row past ``backward_blocks(rows)`` is read, nothing past the reported size is
    written); every result equals the plain wrapper call bit for bit."""
    import seld_native
    case = lc.make_case("gaussian", dtype, rows, d, seed=4)
    want = _run(case, relu, gpu_device)
    seld_native.ensure_init(gpu_device)
    lib = seld_native.load_library()
    n = rows * d
    xbuf, xpat, x = _guarded(n, dtype, gpu_device, nan=True)
    gbuf, gpat, dy = _guarded(n, dtype, gpu_device, nan=True)
    x.copy_(case["x"].view(-1))
    dy.copy_(case["dy"].view(-1))
    ybuf, ypat, y = _guarded(n, dtype, gpu_device)
    dxbuf, dxpat, dx = _guarded(n, dtype, gpu_device)
    sbuf, spat, stats = _guarded(2 * rows, F32, gpu_device)
    wbuf, wpat, dweight = _guarded(d, F32, gpu_device)
    bbuf, bpat, dbias = _guarded(d, F32, gpu_device)
    w, b = case["weight"].to(gpu_device), case["bias"].to(gpu_device)
    reported = int(lib.seld_layernorm_workspace_floats(rows, d))
    assert reported == lc.ol.backward_blocks(rows) * 2 * d
    ws = torch.full((2 * reported,), _NAN[F32], dtype=torch.int32, device=gpu_device)
    torch.cuda.synchronize()
    is_bf16 = int(dtype == BF16)
    rc = lib.seld_layernorm_forward(x.data_ptr(), is_bf16, rows, d, w.data_ptr(), b.data_ptr(), 1e-5, int(relu),
                                    y.data_ptr(), stats.data_ptr(), None)
    assert rc == 0, rc
    rc = lib.seld_layernorm_backward(x.data_ptr(), dy.data_ptr(), is_bf16, rows, d, w.data_ptr(), b.data_ptr(),
                                     stats.data_ptr(), int(relu), dx.data_ptr(), dweight.data_ptr(), dbias.data_ptr(),
                                     ws.data_ptr(), None)
    assert rc == 0, rc
    torch.cuda.synchronize()
    for name, buf, pat, size in (("x", xbuf, xpat, n), ("dy", gbuf, gpat, n), ("y", ybuf, ypat, n), ("dx", dxbuf, dxpat, n),
                                 ("stats", sbuf, spat, 2 * rows), ("dweight", wbuf, wpat, d), ("dbias", bbuf, bpat, d)):
        assert _guards_intact(buf, pat, size), name
    assert bool((ws[reported:] == _NAN[F32]).all())
    assert torch.equal(xbuf[GUARD:GUARD + n].cpu(), _bits(case["x"]).view(-1))          # inputs are not written
    assert torch.equal(gbuf[GUARD:GUARD + n].cpu(), _bits(case["dy"]).view(-1))
    assert torch.equal(_bits(y.view(rows, d).cpu()), _bits(want["y"]))
    assert torch.equal(_bits(dx.view(rows, d).cpu()), _bits(want["dx"]))
    assert torch.equal(_bits(stats.view(rows, 2).cpu()), _bits(want["stats"]))
    assert torch.equal(_bits(dweight.cpu()), _bits(want["dweight"]))
    assert torch.equal(_bits(dbias.cpu()), _bits(want["dbias"]))


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
def test_two_calls_are_bit_identical(gpu_device, dtype):
    case = lc.make_case("near_zero", dtype, 2049, 256, seed=5)
    a, b = _run(case, True, gpu_device), _run(case, True, gpu_device)
    for k in a:
        assert torch.equal(_bits(a[k]), _bits(b[k])), k


# ------------------------------------------------------------------------------------------------- modules

class _Recorder:
    """Swaps seld_native.layernorm_forward / layernorm_backward for recording pass-throughs for a ``with`` block."""

    def __init__(self):
        self.forward, self.backward = [], []

    def __enter__(self):
        import seld_native
        self._native, self._fwd, self._bwd = seld_native, seld_native.layernorm_forward, seld_native.layernorm_backward

        def fwd(x, weight, bias, eps, relu):
            got = self._fwd(x, weight, bias, eps, relu)
            self.forward.append(dict(x=x, weight=weight, bias=bias, eps=eps, relu=relu, y=got[0], stats=got[1]))
            return got

        def bwd(x, dy, weight, bias, stats, relu):
            got = self._bwd(x, dy, weight, bias, stats, relu)
            self.backward.append(dict(x=x, dy=dy, stats=stats, relu=relu, dx=got[0], dweight=got[1], dbias=got[2]))
            return got

        seld_native.layernorm_forward, seld_native.layernorm_backward = fwd, bwd
        return self

    def __exit__(self, *exc):
        self._native.layernorm_forward, self._native.layernorm_backward = self._fwd, self._bwd
        return False


def test_norm_at_d256_under_bf16_autocast(gpu_device):
    """The Conformer blocks' call: D = 256, bf16, a non-contiguous [3, 7, 256] input and an fp32, non-contiguous
    upstream gradient.  The four checks are applied to what the wrapper handed to the kernel."""
    import seld_layernorm
    g = torch.Generator().manual_seed(11)
    ln = nn.LayerNorm(256).to(gpu_device)
    with torch.no_grad():
        ln.weight.copy_(torch.randn(256, generator=g) * 0.5 + 1)
        ln.bias.copy_(torch.randn(256, generator=g) * 0.2)
    x = (torch.randn(7, 3, 256, generator=g) * 2).bfloat16().to(gpu_device).transpose(0, 1).requires_grad_(True)
    go = torch.randn(7, 3, 256, generator=g).to(gpu_device).transpose(0, 1)
    assert x.shape == (3, 7, 256) and not x.is_contiguous() and go.dtype == F32 and not go.is_contiguous()
    was = seld_layernorm.enabled
    try:
        seld_layernorm.enabled = True
        with _Recorder() as rec:
            with torch.autocast("cuda", dtype=BF16):
                y = seld_layernorm.norm(ln, x)
            y.backward(go)
    finally:
        seld_layernorm.enabled = was
    torch.cuda.synchronize()
    assert len(rec.forward) == 1 and len(rec.backward) == 1
    f, b = rec.forward[0], rec.backward[0]
    assert f["x"].dtype == BF16 and f["x"].is_contiguous() and f["relu"] is False and y.dtype == BF16
    assert b["dy"].dtype == BF16 and b["dy"].is_contiguous() and b["dy"].shape == f["x"].shape
    assert torch.equal(_bits(f["x"].cpu()), _bits(x.detach().contiguous().cpu()))
    assert torch.equal(_bits(b["dy"].cpu()), _bits(go.bfloat16().contiguous().cpu()))
    case = dict(x=f["x"].reshape(-1, 256).cpu(), dy=b["dy"].reshape(-1, 256).cpu(), weight=f["weight"].detach().cpu(),
                bias=f["bias"].detach().cpu(), eps=f["eps"])
    out = dict(y=f["y"].reshape(-1, 256).cpu(), stats=f["stats"].cpu(), dx=b["dx"].reshape(-1, 256).cpu(),
               dweight=b["dweight"].cpu(), dbias=b["dbias"].cpu())
    _report("norm D=256 bf16 autocast", case, out, False)
    assert torch.equal(_bits(y.detach().cpu()), _bits(f["y"].cpu()))
    assert x.grad.shape == x.shape and torch.equal(_bits(x.grad.contiguous().cpu()), _bits(b["dx"].cpu()))
    assert torch.equal(ln.weight.grad, b["dweight"]) and torch.equal(ln.bias.grad, b["dbias"])


def test_layernorm_function_on_every_path_the_models_use(gpu_device):
    """``_LayerNorm`` after the wrappers learnt to refuse: the head path (relu, 3-D input, fp32 and bf16), a
    non-contiguous input, an expanded (stride-0) upstream gradient as ``sum().backward()`` delivers it."""
    import seld_layernorm
    torch.manual_seed(12)
    for d, dtype, relu in ((512, F32, True), (1024, BF16, True), (256, BF16, False), (2048, F32, False)):
        ln = nn.LayerNorm(d).to(gpu_device)
        x = torch.randn(5, 2, d, device=gpu_device).to(dtype).transpose(0, 1).requires_grad_(True)
        with _Recorder() as rec:
            y = seld_layernorm.layer_norm(ln, x, relu=relu)
            y.float().sum().backward()
        assert len(rec.forward) == 1 and len(rec.backward) == 1
        ref = torch.nn.functional.layer_norm(x.detach().double(), (d,), ln.weight.double(), ln.bias.double(), ln.eps)
        ref = torch.relu(ref) if relu else ref
        tol = (2.0 ** -8 if dtype == BF16 else 2e-5) * ref.abs().max().item()
        assert (y.double() - ref).abs().max().item() <= tol
        assert x.grad is not None and ln.weight.grad is not None and ln.bias.grad is not None
        assert bool(torch.isfinite(x.grad.float()).all())


def test_conformer_conv_module_reaches_the_fused_kernel(gpu_device):
    import seld_dwconv
    import seld_layernorm
    from model_conformer import ConformerConvModule
    torch.manual_seed(13)
    module = ConformerConvModule(256, kernel_size=31, dropout=0.0).to(gpu_device)
    x = torch.randn(2, 20, 256, device=gpu_device, requires_grad=True)
    was = seld_dwconv.enabled, seld_layernorm.enabled
    try:
        seld_dwconv.enabled = seld_layernorm.enabled = True
        assert seld_dwconv.applicable(module, x)
        with _Recorder() as rec:
            with torch.autocast("cuda", dtype=BF16):
                y = module(x)
            y.float().square().mean().backward()
    finally:
        seld_dwconv.enabled, seld_layernorm.enabled = was
    assert len(rec.forward) == 1 and len(rec.backward) == 1
    assert rec.forward[0]["x"].shape[-1] == 256 and rec.forward[0]["relu"] is False
    assert module.layer_norm.weight.grad is not None and x.grad is not None


# ------------------------------------------------------------------------------------------------- refusals

def test_wrappers_refuse_bad_device_arguments(gpu_device):
    """Each refusal happens before a launch: the outputs of a good call made before are what a good call makes after."""
    import seld_native
    dev = gpu_device
    good = dict(x=torch.randn(3, 256, device=dev), dy=torch.randn(3, 256, device=dev), weight=torch.ones(256, device=dev),
                bias=torch.zeros(256, device=dev))
    y, stats = seld_native.layernorm_forward(good["x"], good["weight"], good["bias"], 1e-5, True)
    bad_forward = {
        "x not contiguous": dict(x=torch.randn(256, 3, device=dev).t()),
        "weight bf16": dict(weight=good["weight"].bfloat16()),
        "bias float64": dict(bias=good["bias"].double()),
        "weight strided": dict(weight=torch.ones(512, device=dev)[::2]),
        "bias strided": dict(bias=torch.ones(512, device=dev)[::2]),
        "weight length": dict(weight=torch.ones(512, device=dev)),
        "bias length": dict(bias=torch.ones(128, device=dev)),
        "weight on the host": dict(weight=torch.ones(256)),
        "bias on the host": dict(bias=torch.zeros(256)),
    }
    bad_backward = {
        "dy bf16": dict(dy=good["dy"].bfloat16()),
        "dy shape": dict(dy=torch.randn(2, 256, device=dev)),
        "dy not contiguous": dict(dy=torch.randn(256, 3, device=dev).t()),
        "dy on the host": dict(dy=torch.randn(3, 256)),
        "stats float64": dict(stats=stats.double()),
        "stats flat": dict(stats=stats.reshape(-1)),
        "stats rows": dict(stats=stats[:2].contiguous()),
        "stats strided": dict(stats=torch.zeros(3, 4, device=dev)[:, ::2]),
        "stats on the host": dict(stats=stats.cpu()),
    }
    for name, change in bad_forward.items():
        a = dict(good, **change)
        with pytest.raises(seld_native.SeldNativeError, match="layernorm_forward"):
            seld_native.layernorm_forward(a["x"], a["weight"], a["bias"], 1e-5, True)
        with pytest.raises(seld_native.SeldNativeError, match="layernorm_backward"):
            seld_native.layernorm_backward(a["x"], a["dy"], a["weight"], a["bias"], stats, True)
    for name, change in bad_backward.items():
        a = dict(dict(good, stats=stats), **change)
        with pytest.raises(seld_native.SeldNativeError, match="layernorm_backward"):
            seld_native.layernorm_backward(a["x"], a["dy"], a["weight"], a["bias"], a["stats"], True)
    y2, stats2 = seld_native.layernorm_forward(good["x"], good["weight"], good["bias"], 1e-5, True)
    assert torch.equal(y, y2) and torch.equal(stats, stats2)
    seld_native.layernorm_backward(good["x"], good["dy"], good["weight"], good["bias"], stats, True)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------- summary

def test_zz_worst_ratios_of_the_module():
    """Printed last: the worst error / bound ratio of every check over all cases above, and the worst rsqrtf distance
    (the figure RSQRT_MEASURED in tests/layernorm_checks.py records)."""
    print("\nworst ratios: " + lc.fmt(WORST))
    print(f"worst rsqrtf distance: {RSQRT[0]:.4f} ulp (allowance {lc.RSQRT_ULPS})")
    assert RSQRT[0] <= lc.RSQRT_MEASURED, "rsqrtf is further from the correctly rounded value than recorded"
