"""GPU checks of the 3x3-convolution forward kernel with the BatchNorm statistics epilogue (csrc/convfwd.hip,
seld_native.conv3x3_forward, seld_native.conv_tail_forward_from_partials) that model_crnn.ConvBlock uses in training for
the encoder's adopted blocks in place of the library convolution and the tail's statistics pass.

Reference: float64 conv2d on the same bf16 values (CPU, tests/conv_fwd_cases.py).  The bar per element is one bf16
rounding of the result plus a worst-case fp32 accumulation over K = 9 * Cin terms in any order:

    |got - ref| <= 2^-8 |ref| + 2 * 9 * Cin * 2^-24 * S,      S = the same convolution of |x| and |w|

No measured constant enters it.

Measured on an MI355X (the figures the tests print): worst error / bound of the convolution 0.80 .. 0.91 over the six
shapes.  Statistics against float64 sums of the stored y, largest over the channels, per shape: the epilogue's partial
rows 0 .. 1.9e-6 (sum) and 3.0e-7 .. 9.8e-5 (sum of squares, 6.3e-8 .. 1.2e-7 relative); the sums that the mean and
1/sigma of the existing statistics pass stand for 0 .. 3.9e-6 and 1.0e-6 .. 4.2e-4.  ConvBlock: pooled outputs 0.31 of
their tolerance, running_mean 5.8e-10 against 7.7e-10, running_var 6.4e-8 against 8.8e-8.
"""
import pytest
import torch
import torch.nn.functional as F

import conv_fwd_cases as cases

pytestmark = pytest.mark.gpu
K_ERR_UNSUPPORTED = -4                  # include/seld_hip.h


def _on_device(x, device):
    return x.to(device).contiguous(memory_format=torch.channels_last)


def _worst(got, ref, bound):
    err = (got.double().cpu() - ref).abs()
    return (err / (bound + 1e-300)).max().item(), err.max().item()


def _ulp32(v):
    """One fp32 ulp of |v| (float64 tensor in and out)."""
    v = v.abs().clamp_min(2.0 ** -126)
    return 2.0 ** (torch.floor(torch.log2(v)) - 23)


@pytest.mark.parametrize("b,t,f,cin,cout", cases.SHAPES)
def test_matches_float64_convolution(gpu_device, b, t, f, cin, cout):
    import seld_native
    x, w, ref, mag = cases.case(b, t, f, cin, cout)
    xd, wd = _on_device(x, gpu_device), _on_device(w, gpu_device)
    assert seld_native.conv3x3_forward_applicable(xd, wd)
    y = seld_native.conv3x3_forward(xd, wd)
    ys, _ = seld_native.conv3x3_forward(xd, wd, stats=True)
    torch.cuda.synchronize()
    assert y.shape == (b, cout, t, f) and y.dtype == torch.bfloat16
    assert y.is_contiguous(memory_format=torch.channels_last)
    assert torch.equal(y, ys)                                           # the epilogue does not change what is stored
    worst, err = _worst(y, ref, cases.bound(ref, mag, cin))
    print(f"\n{(b, t, f, cin, cout)}: worst error / bound {worst:.3f}, max abs error {err:.3e}")
    assert worst <= 1.0, (worst, err, ref.abs().max().item())


@pytest.mark.parametrize("b,t,f,cin,cout", cases.SHAPES)
def test_partial_rows_sum_to_the_stored_values(gpu_device, b, t, f, cin, cout):
    """One partial row per chunk; summed over the rows, the sum and the sum of squares per channel agree with float64
    sums of the y the kernel stored.  Allowed: twice the error of the existing statistics (the sums that the mean and
    1/sigma returned by conv_tail_forward on the same y stand for, largest over the channels), at least one fp32 ulp of
    the quantity."""
    import seld_native
    x, w, _, _ = cases.case(b, t, f, cin, cout)
    y, partials = seld_native.conv3x3_forward(_on_device(x, gpu_device), _on_device(w, gpu_device), stats=True)
    eps = 1e-5
    # the tail takes channel counts 8 * (a divisor of 256): 192 channels go through it as three 64-channel slices of the
    # same values (the statistics are per channel)
    step = cout if seld_native.conv_tail_supported(cout) else 64
    pieces = []
    for c0 in range(0, cout, step):
        ones, zeros = torch.ones(step, device=gpu_device), torch.zeros(step, device=gpu_device)
        ys = y[:, c0:c0 + step].contiguous(memory_format=torch.channels_last)
        pieces.append(seld_native.conv_tail_forward(ys, ones, zeros, zeros.clone(), ones.clone(), 0.1, eps, True, 2)[1])
    mean_invstd = torch.cat(pieces, dim=1)
    torch.cuda.synchronize()
    assert tuple(partials.shape) == (2, cases.chunks(b, t, f), cout)
    yd = y.double().cpu()
    n = b * t * f
    want = torch.stack([yd.sum((0, 2, 3)), (yd * yd).sum((0, 2, 3))])
    got = partials.double().cpu().sum(1)
    mean, invstd = mean_invstd.double().cpu()
    existing = torch.stack([n * mean, n * (1.0 / (invstd * invstd) - eps + mean * mean)])
    for s, name in enumerate(("sum", "sum of squares")):
        err_new, err_old = (got[s] - want[s]).abs(), (existing[s] - want[s]).abs()
        allowed = torch.maximum(2 * err_old.max(), _ulp32(want[s]))
        rel = (err_new / want[s].abs().clamp_min(1e-30)).max().item()
        print(f"\n{(b, t, f, cin, cout)} {name}: epilogue max abs error {err_new.max().item():.3e} (rel {rel:.2e}), "
              f"existing pass {err_old.max().item():.3e}")
        assert (err_new <= allowed).all(), (name, err_new.max().item(), err_old.max().item())


def test_integer_case_matches_the_statistics_pass(gpu_device):
    """Integer-valued y (exact in bf16, every fp32 partial sum exact; tests/test_conv_fwd_cpu.py asserts the premise) at
    a ragged shape: the tail fed from the partial rows returns the statistics pass's mean, 1/sigma and coefficients to
    1 fp32 ulp and the same pooled output.  A padded position leaking into the sums would show here."""
    import seld_native
    x, w, ref = cases.integer_case()
    cout = w.shape[0]
    y, partials = seld_native.conv3x3_forward(_on_device(x, gpu_device), _on_device(w, gpu_device), stats=True)
    assert torch.equal(y.double().cpu(), ref)
    g = torch.Generator(device="cpu").manual_seed(78)
    gamma = (torch.rand(cout, generator=g) + 0.5).to(gpu_device)
    beta = torch.randn(cout, generator=g).to(gpu_device)
    zeros, ones = torch.zeros(cout, device=gpu_device), torch.ones(cout, device=gpu_device)
    rm_a, rv_a, rm_b, rv_b = zeros.clone(), ones.clone(), zeros.clone(), ones.clone()
    out_a, mi_a, ss_a = seld_native.conv_tail_forward(y, gamma, beta, rm_a, rv_a, 0.1, 1e-5, True, 2)
    out_b, mi_b, ss_b = seld_native.conv_tail_forward_from_partials(y, partials, gamma, beta, rm_b, rv_b, 0.1, 1e-5, 2)
    torch.cuda.synchronize()
    yd = ref
    assert torch.equal(partials.double().cpu().sum(1), torch.stack([yd.sum((0, 2, 3)), (yd * yd).sum((0, 2, 3))]))
    for a, b_ in ((mi_a, mi_b), (ss_a, ss_b), (rm_a, rm_b), (rv_a, rv_b)):
        a, b_ = a.double().cpu(), b_.double().cpu()
        assert ((a - b_).abs() <= _ulp32(a)).all(), (a - b_).abs().max().item()
    assert torch.equal(out_a, out_b)


def test_nothing_crosses_a_clip_boundary(gpu_device):
    """x is non-zero only in the last time row of clip 0: clip 1's y and its partial rows are exactly zero."""
    import seld_native
    b, t, f, cin, cout = 2, 5, 8, 64, 64
    x, w = cases.inputs(b, t, f, cin, cout, seed=11)
    x = x.clone()
    x[1] = 0
    x[0, :, :t - 1] = 0
    y, partials = seld_native.conv3x3_forward(_on_device(x, gpu_device), _on_device(w, gpu_device), stats=True)
    torch.cuda.synchronize()
    assert torch.count_nonzero(y[0]).item() > 0
    assert torch.count_nonzero(y[1]).item() == 0
    assert torch.count_nonzero(partials[:, 0]).item() > 0 and torch.count_nonzero(partials[:, 1]).item() == 0
    ref, mag = cases.reference(x, w)
    assert _worst(y, ref, cases.bound(ref, mag, cin))[0] <= 1.0


@pytest.mark.parametrize("f", [8, 16, 32])
@pytest.mark.parametrize("edge", ["last", "first"])
def test_nothing_wraps_round_a_frequency_edge(gpu_device, f, edge):
    """x is non-zero only in the last (first) frequency column: y is exactly zero beyond the neighbouring column, in
    particular in the first (last) column of the next (previous) time row, where a wrap-around would land."""
    import seld_native
    b, t, cin, cout = 2, 4, 64, 64
    x, w = cases.inputs(b, t, f, cin, cout, seed=12 + f)
    x = x.clone()
    keep = f - 1 if edge == "last" else 0
    mask = torch.zeros(f, dtype=torch.bool)
    mask[keep] = True
    x[..., ~mask] = 0
    y = seld_native.conv3x3_forward(_on_device(x, gpu_device), _on_device(w, gpu_device))
    torch.cuda.synchronize()
    far = y[..., :f - 2] if edge == "last" else y[..., 2:]
    near = y[..., f - 2:] if edge == "last" else y[..., :2]
    assert torch.count_nonzero(far).item() == 0
    assert torch.count_nonzero(near).item() > 0
    ref, mag = cases.reference(x, w)
    assert _worst(y, ref, cases.bound(ref, mag, cin))[0] <= 1.0


@pytest.mark.parametrize("b,t,f,cin,cout", [(2, 17, 8, 64, 64), (1, 9, 32, 64, 128), (2, 3, 16, 128, 192)])
def test_writes_nothing_outside_y_and_the_partial_rows(gpu_device, b, t, f, cin, cout):
    """y and the partial rows are slices of larger buffers of a sentinel pattern with guards before and after (T is not
    a multiple of the time rows per chunk: the ragged last chunk of every clip): the guards come back bit-identical."""
    import seld_native
    x, w = cases.inputs(b, t, f, cin, cout)
    ref, mag = cases.reference(x, w)
    guard, n = 64 * cout, b * t * f * cout
    pattern = (torch.arange(n + 2 * guard, dtype=torch.int32) % 251 + 0x3F00).to(torch.int16).to(gpu_device)
    buf = pattern.clone()
    out = buf[guard:guard + n].view(torch.bfloat16).view(b, t, f, cout).permute(0, 3, 1, 2)
    rows = cases.chunks(b, t, f)
    pguard, pn = 4 * cout, 2 * rows * cout
    ppattern = (torch.arange(pn + 2 * pguard, dtype=torch.float32) % 253 + 1000.0).to(gpu_device)
    pbuf = ppattern.clone()
    pout = pbuf[pguard:pguard + pn].view(2, rows, cout)
    y, partials = seld_native.conv3x3_forward(_on_device(x, gpu_device), _on_device(w, gpu_device), stats=True, out=out,
                                              partials=pout)
    torch.cuda.synchronize()
    assert y.data_ptr() == out.data_ptr() and partials.data_ptr() == pout.data_ptr()
    assert torch.equal(buf[:guard], pattern[:guard]) and torch.equal(buf[guard + n:], pattern[guard + n:])
    assert torch.equal(pbuf[:pguard], ppattern[:pguard]) and torch.equal(pbuf[pguard + pn:], ppattern[pguard + pn:])
    assert _worst(y, ref, cases.bound(ref, mag, cin))[0] <= 1.0


def test_two_calls_are_bit_identical(gpu_device):
    import seld_native
    x, w = cases.inputs(3, 40, 16, 128, 128, seed=14)
    xd, wd = _on_device(x, gpu_device), _on_device(w, gpu_device)
    a, pa = seld_native.conv3x3_forward(xd, wd, stats=True)
    b, pb = seld_native.conv3x3_forward(xd, wd, stats=True)
    torch.cuda.synchronize()
    assert torch.equal(a, b) and torch.equal(pa, pb)


@pytest.mark.parametrize("f,cin,cout", [(64, 64, 64), (8, 4, 64), (8, 96, 64), (8, 64, 32), (16, 64, 96)])
def test_unsupported_shapes_are_refused(gpu_device, f, cin, cout):
    import seld_native
    x, w = cases.inputs(1, 2, f, cin, cout, seed=15)
    xd, wd = _on_device(x, gpu_device), _on_device(w, gpu_device)
    assert not seld_native.conv3x3_forward_applicable(xd, wd)
    with pytest.raises(seld_native.SeldNativeError):
        seld_native.conv3x3_forward(xd, wd)
    seld_native.ensure_init(gpu_device)
    y = torch.empty(1, cout, 2, f, dtype=torch.bfloat16, device=gpu_device).contiguous(memory_format=torch.channels_last)
    lib = seld_native.load_library()
    rc = lib.seld_conv3x3_forward(xd.data_ptr(), wd.data_ptr(), 1, 2, f, cin, cout, y.data_ptr(), None, None)
    assert rc == K_ERR_UNSUPPORTED, rc


def test_conv_block_with_and_without_the_kernel(gpu_device):
    """ConvBlock(64, 128) under bf16 autocast at (B, T, F) = (2, 9, 32) with FUSED_CONV_FWD on and off.

    * the two convolution outputs (what each tail received) lie within twice the float64 bound of each other;
    * the pooled outputs are compared where the float64 reference puts both pre-activations of the pair farther from the
      ReLU and from each other than that difference allows (tests/test_conv_fwd_cpu.py: under 2 % are left out).  max and
      ReLU are 1-Lipschitz, so there |out_on - out_off| <= |a| * 2 * bound (the larger of the pair) + two bf16
      roundings of z (2 * 2^-8 |z|) + 2^-8 |z| for the 1e-6-level difference of the coefficients;
    * the upstream gradient is zero on the left-out elements, so both passes route it alike.  Each pass's input and weight
      gradient is held to the data-gradient and weight-gradient tests' own bars, against references formed from the dy
      that pass handed its convolution backward; the two passes' gradients then differ by no more than those bars plus
      the same (linear) backward of the measured difference of their dy;
    * the running statistics of each pass match float64 statistics of the y its tail received, to the tolerance of the
      partial-rows test (twice the existing pass's error, at least one fp32 ulp)."""
    import model_crnn
    import seld_native
    c = cases.block_case()
    b, t, f, cin, cout = cases.BLOCK_SHAPE
    safe = cases.block_safe_mask(c)
    assert 1.0 - safe.double().mean().item() <= 0.02
    block = model_crnn.ConvBlock(cin, cout, pool_size=(1, 2))
    with torch.no_grad():
        block.conv.weight.copy_(c["w"])
        block.bn.weight.copy_(c["gamma"])
        block.bn.bias.copy_(c["beta"])
    block = block.to(gpu_device).to(memory_format=torch.channels_last).train()
    g = torch.Generator(device="cpu").manual_seed(6)
    gy = (torch.randn(b, cout, t, f // 2, generator=g) * safe).to(torch.bfloat16)
    gy = _on_device(gy, gpu_device)

    tails, dgrads, wgrads = [], [], []
    real = (seld_native.conv_tail_forward, seld_native.conv_tail_forward_from_partials, seld_native.conv3x3_dgrad,
            seld_native.conv3x3_wgrad)

    def tail(x, *a, **k):
        tails.append(("stats", x.detach().clone()))
        return real[0](x, *a, **k)

    def tail_partials(x, *a, **k):
        tails.append(("partials", x.detach().clone()))
        return real[1](x, *a, **k)

    def dgrad(dy, w, out=None):
        dgrads.append((dy.detach().clone(), w.detach().clone()))
        return real[2](dy, w, out)

    def wgrad(x, dy, dw):
        wgrads.append((x.detach().clone(), dy.detach().clone()))
        return real[3](x, dy, dw)

    was = model_crnn.ConvBlock.fused_fwd
    res = {}
    try:
        (seld_native.conv_tail_forward, seld_native.conv_tail_forward_from_partials, seld_native.conv3x3_dgrad,
         seld_native.conv3x3_wgrad) = tail, tail_partials, dgrad, wgrad
        for on in (True, False):
            model_crnn.ConvBlock.fused_fwd = on
            with torch.no_grad():
                block.bn.running_mean.zero_()
                block.bn.running_var.fill_(1.0)
            x = _on_device(c["x"], gpu_device).requires_grad_(True)
            with torch.autocast(device_type="cuda", dtype=torch.bfloat16):
                out = block(x)
            dx, dw = torch.autograd.grad(out, (x, block.conv.weight), gy)
            torch.cuda.synchronize()
            res[on] = {"out": out.detach(), "dx": dx, "dw": dw, "rm": block.bn.running_mean.clone(),
                       "rv": block.bn.running_var.clone()}
    finally:
        (seld_native.conv_tail_forward, seld_native.conv_tail_forward_from_partials, seld_native.conv3x3_dgrad,
         seld_native.conv3x3_wgrad) = real
        model_crnn.ConvBlock.fused_fwd = was
    assert [k for k, _ in tails] == ["partials", "stats"]               # each pass took its own path
    assert len(dgrads) == 2 and len(wgrads) == 2
    y_on, y_off = tails[0][1].double().cpu(), tails[1][1].double().cpu()

    # convolution outputs
    assert ((y_on - c["y"]).abs() <= c["bound"]).all()
    assert ((y_on - y_off).abs() <= 2 * c["bound"]).all()

    # pooled outputs on the safe elements
    a4, b4 = c["a"].view(1, -1, 1, 1), c["b"].view(1, -1, 1, 1)
    z = a4 * c["y"] + b4
    m = a4.abs() * 2 * c["bound"]
    tol = torch.maximum(m[..., 0::2], m[..., 1::2]) + 3 * 2.0 ** -8 * torch.maximum(z[..., 0::2].abs(), z[..., 1::2].abs())
    diff = (res[True]["out"].double() - res[False]["out"].double()).abs().cpu()
    print(f"\npooled outputs: worst difference / tolerance on the safe elements {(diff / tol)[safe].max().item():.3f}")
    assert (diff[safe] <= tol[safe]).all()

    # gradients: each pass against references of its own dy, then against each other
    args = ((1, 1), (1, 1), (1, 1), False, (0, 0), 1, (False, True, False))
    dxs, dws, dx_bounds, dw_bounds = [], [], [], []
    for i, on in enumerate((True, False)):
        dy, w = (v.cpu() for v in dgrads[i])
        wt = w.double().transpose(0, 1).flip(2, 3)
        ref, mag = F.conv2d(dy.double(), wt, padding=1), F.conv2d(dy.double().abs(), wt.abs(), padding=1)
        dx_bound = 2.0 ** -8 * ref.abs() + 2 * 9 * cout * 2.0 ** -24 * mag
        assert ((res[on]["dx"].double().cpu() - ref).abs() <= dx_bound).all(), on
        xs, dyw = wgrads[i]
        wref = torch.ops.aten.convolution_backward(dyw.float(), xs.float(), w.to(gpu_device).float(), None, *args)[1]
        wmag = torch.ops.aten.convolution_backward(dyw.float().abs(), xs.float().abs(), w.to(gpu_device).float(), None,
                                                   *args)[1]
        dw_bound = 1e-5 * wmag + 1e-30                                   # fp32 weight gradient: no rounding term
        assert res[on]["dw"].dtype == torch.float32
        assert ((res[on]["dw"] - wref).abs() <= dw_bound).all(), on
        dxs.append(ref), dws.append(wref), dx_bounds.append(dx_bound), dw_bounds.append(dw_bound)
    ddy = (dgrads[0][0].double() - dgrads[1][0].double()).abs()
    wt = dgrads[0][1].double().transpose(0, 1).flip(2, 3).abs()
    spread = F.conv2d(ddy.cpu(), wt.cpu(), padding=1)
    assert ((res[True]["dx"].double() - res[False]["dx"].double()).abs().cpu()
            <= dx_bounds[0] + dx_bounds[1] + spread).all()
    wspread = torch.ops.aten.convolution_backward(ddy.float(), wgrads[0][0].float().abs(), res[True]["dw"], None, *args)[1]
    assert ((res[True]["dw"] - res[False]["dw"]).abs() <= dw_bounds[0] + dw_bounds[1] + wspread * (1 + 1e-5)).all()

    # running statistics of each pass against float64 statistics of the y its tail received
    n = b * t * f
    errs = {}
    for on, y in ((True, y_on), (False, y_off)):
        want_m = 0.1 * y.mean((0, 2, 3))
        want_v = 0.9 + 0.1 * y.var((0, 2, 3), unbiased=True)
        errs[on] = ((res[on]["rm"].double().cpu() - want_m).abs(), (res[on]["rv"].double().cpu() - want_v).abs(),
                    want_m, want_v)
    for k, name in ((0, "running_mean"), (1, "running_var")):
        allowed = torch.maximum(2 * errs[False][k].max(), _ulp32(errs[True][2 + k]))
        print(f"{name}: epilogue path max error {errs[True][k].max().item():.3e}, statistics pass "
              f"{errs[False][k].max().item():.3e}")
        assert (errs[True][k] <= allowed).all(), name
