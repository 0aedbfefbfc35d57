"""The depthwise Conv1d kernels (csrc/dwconv.hip) against the float64 restatement of oracle/dwconv.py on the same bf16 or
fp32 values: forward with and without bias, the flipped-tap data gradient, the weight / bias gradient, in both dtypes,
at the time extents where the 32-step forward block and the 50-step weight-gradient chunk begin and end.

Bounds (tests/tail_checks.py; the form of tests/test_conv_dgrad_gpu.py), S = the magnitude sum of the terms:
    outputs             |err| <= rho |ref| + 2 K 2^-24 S        rho = 2^-8 for bf16 outputs, 0 for fp32
    dweight, dbias      |err| <= (B T + 4) 2^-24 S
Each test prints its worst error / bound ratios.
"""
import pytest
import torch

import tail_checks as tc
from oracle import dwconv as od

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float32]
K_UNSUPPORTED = -4                                                     # kErrUnsupported (include/seld_hip.h)

# (B, T, D, K): T <= pad (1, 15), T = pad + 1, T around the 32-step block (31, 32, 33) and the 50-step chunk
# (49, 50, 51), two and three chunks with a ragged last one (99, 101), the production shape (250, 512, 31), K = 1 and 3
SHAPES = [(1, 1, 64, 31), (2, 15, 64, 31), (2, 16, 128, 31), (3, 31, 64, 31), (1, 32, 64, 7), (2, 33, 128, 31),
          (2, 49, 64, 31), (2, 50, 64, 15), (3, 51, 128, 31), (1, 99, 64, 3), (2, 101, 512, 31), (2, 250, 512, 31),
          (2, 37, 64, 1)]


def _inputs(b, t, d, k, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(b, t, d, generator=g).to(dtype)
    dy = torch.randn(b, t, d, generator=g).to(dtype)
    return x, dy, torch.randn(d, k, generator=g) * 0.2, torch.randn(d, generator=g)


def _grad_ratios(dw, db, x, dy, k):
    b, t, _ = x.shape
    rw, mw, rb, mb = od.wgrad(x, dy, k)
    return {"dweight": tc.dw_grad_ratio(dw.cpu(), rw, mw, b, t), "dbias": tc.dw_grad_ratio(db.cpu(), rb, mb, b, t)}


def _report(what, ratios):
    print(f"\n{what}: {tc.fmt(ratios)}")
    assert tc.passes(ratios), tc.fmt(ratios)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
@pytest.mark.parametrize("b,t,d,k", SHAPES)
def test_matches_float64_restatement(gpu_device, b, t, d, k, dtype):
    import seld_native
    x, dy, w, bias = _inputs(b, t, d, k, dtype, seed=1000 * t + d + k)
    xd, dyd, wd, bd = (v.to(gpu_device) for v in (x, dy, w, bias))
    y = seld_native.dwconv1d(xd, wd, bd)
    y0 = seld_native.dwconv1d(xd, wd, None)
    dx = seld_native.dwconv1d(dyd, wd, None, flip=True)
    dw, db = seld_native.dwconv1d_wgrad(xd, dyd, k)
    torch.cuda.synchronize()
    assert y.dtype == dtype and dx.dtype == dtype and dw.dtype == torch.float32 and dw.shape == (d, k) and db.shape == (d,)
    ratios = {"y": tc.dw_output_ratio(y.cpu(), *od.forward(x, w, bias), k),
              "y_no_bias": tc.dw_output_ratio(y0.cpu(), *od.forward(x, w, None), k),
              "dx": tc.dw_output_ratio(dx.cpu(), *od.dgrad(dy, w), k)}
    ratios.update(_grad_ratios(dw, db, x, dy, k))
    _report(f"{(b, t, d, k)}", ratios)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
def test_nothing_crosses_a_batch_boundary(gpu_device, dtype):
    """x (dy) non-zero only in batch row 0: batch row 1 of y (dx) is exactly zero without a bias, and with dy zero in
    batch row 1 the parameter gradients are those of batch row 0 alone."""
    import seld_native
    b, t, d, k = 2, 33, 64, 31
    x, dy, w, _ = _inputs(b, t, d, k, dtype, seed=21)
    x0, dy0 = x.clone(), dy.clone()
    x0[1], dy0[1] = 0, 0
    wd = w.to(gpu_device)
    y = seld_native.dwconv1d(x0.to(gpu_device), wd, None)
    dx = seld_native.dwconv1d(dy0.to(gpu_device), wd, None, flip=True)
    dw, db = seld_native.dwconv1d_wgrad(x.to(gpu_device), dy0.to(gpu_device), k)        # x keeps its batch row 1
    dw1, db1 = seld_native.dwconv1d_wgrad(x[:1].to(gpu_device), dy[:1].to(gpu_device), k)
    torch.cuda.synchronize()
    assert torch.count_nonzero(y[0]).item() > 0 and torch.count_nonzero(y[1]).item() == 0
    assert torch.count_nonzero(dx[0]).item() > 0 and torch.count_nonzero(dx[1]).item() == 0
    assert torch.equal(dw, dw1) and torch.equal(db, db1)
    ratios = {"y": tc.dw_output_ratio(y.cpu(), *od.forward(x0, w, None), k),
              "dx": tc.dw_output_ratio(dx.cpu(), *od.dgrad(dy0, w), k)}
    ratios.update(_grad_ratios(dw, db, x, dy0, k))
    _report("batch isolation", ratios)


@pytest.mark.parametrize("t", [33, 51])
def test_writes_nothing_outside_y_and_partial(gpu_device, t):
    """y and the weight-gradient partial buffer are slices of sentinel-filled buffers, passed to the C ABI by address:
    the guards come back bit-identical and the slices hold what the wrappers return."""
    import seld_native
    b, d, k, dtype = 2, 64, 31, torch.bfloat16
    x, dy, w, bias = _inputs(b, t, d, k, dtype, seed=31)
    xd, dyd, wd, bd = (v.to(gpu_device).contiguous() for v in (x, dy, w, bias))
    want_y = seld_native.dwconv1d(xd, wd, bd)
    want_dw, want_db = seld_native.dwconv1d_wgrad(xd, dyd, k)
    lib = seld_native.load_library()
    n, guard = b * t * d, 64 * d
    ypat = (torch.arange(n + 2 * guard, dtype=torch.int32) % 251 + 0x3F00).to(torch.int16).to(gpu_device)
    ybuf = ypat.clone()
    y = ybuf[guard:guard + n].view(torch.bfloat16)
    rows = int(lib.seld_dwconv1d_wgrad_rows(b, t))
    assert rows == b * ((t + 49) // 50)
    m = rows * d * 32
    ppat = (torch.arange(m + 2 * guard, dtype=torch.float32) % 251 + 1000.0).to(gpu_device)
    pbuf = ppat.clone()
    partial = pbuf[guard:guard + m]
    torch.cuda.synchronize()
    assert lib.seld_dwconv1d(xd.data_ptr(), 1, wd.data_ptr(), bd.data_ptr(), b, t, d, k, 0, y.data_ptr(), None) == 0
    assert lib.seld_dwconv1d_wgrad(xd.data_ptr(), dyd.data_ptr(), 1, b, t, d, k, partial.data_ptr(), None) == 0
    torch.cuda.synchronize()
    assert torch.equal(ybuf[:guard], ypat[:guard]) and torch.equal(ybuf[guard + n:], ypat[guard + n:])
    assert torch.equal(pbuf[:guard], ppat[:guard]) and torch.equal(pbuf[guard + m:], ppat[guard + m:])
    assert torch.equal(y.view(b, t, d).view(torch.int16), want_y.view(torch.int16))
    total = partial.view(rows, d, 32).sum(0)
    assert torch.equal(total[:, :k], want_dw) and torch.equal(total[:, 31], want_db)


@pytest.mark.parametrize("d,k", [(64, 30), (64, 33), (96, 31)])
def test_unsupported_shapes_are_refused_and_write_nothing(gpu_device, d, k):
    import seld_native
    b, t = 2, 33
    assert not seld_native.dwconv1d_supported(d, k)
    x = torch.randn(b, t, d, device=gpu_device).to(torch.bfloat16)
    w = torch.randn(d, k, device=gpu_device)
    with pytest.raises(seld_native.SeldNativeError):
        seld_native.dwconv1d(x, w, None)
    with pytest.raises(seld_native.SeldNativeError):
        seld_native.dwconv1d_wgrad(x, x, k)
    seld_native.ensure_init(gpu_device)
    lib = seld_native.load_library()
    y = torch.full((b, t, d), 3.0, dtype=torch.bfloat16, device=gpu_device)
    partial = torch.full((2 * b, d, 32), 7.0, device=gpu_device)
    torch.cuda.synchronize()
    rc = lib.seld_dwconv1d(x.data_ptr(), 1, w.data_ptr(), None, b, t, d, k, 0, y.data_ptr(), None)
    assert rc == K_UNSUPPORTED, rc
    rc = lib.seld_dwconv1d_wgrad(x.data_ptr(), x.data_ptr(), 1, b, t, d, k, partial.data_ptr(), None)
    assert rc == K_UNSUPPORTED, rc
    torch.cuda.synchronize()
    assert (y == 3.0).all().item() and (partial == 7.0).all().item()


def test_autograd_under_bf16_activations(gpu_device):
    """_DepthwiseConv1d with bf16 activations and fp32 parameters, the configuration the wide Conformer trains in."""
    from seld_dwconv import _DepthwiseConv1d
    b, t, d, k = 2, 101, 512, 31
    x, dy, w, bias = _inputs(b, t, d, k, torch.bfloat16, seed=41)
    xd = x.to(gpu_device).requires_grad_(True)
    wd = w.to(gpu_device).reshape(d, 1, k).requires_grad_(True)
    bd = bias.to(gpu_device).requires_grad_(True)
    y = _DepthwiseConv1d.apply(xd, wd, bd)
    y.backward(dy.to(gpu_device))
    torch.cuda.synchronize()
    assert y.dtype == torch.bfloat16 and xd.grad.dtype == torch.bfloat16
    assert wd.grad.dtype == torch.float32 and wd.grad.shape == (d, 1, k) and bd.grad.dtype == torch.float32
    ratios = {"y": tc.dw_output_ratio(y.detach().cpu(), *od.forward(x, w, bias), k),
              "dx": tc.dw_output_ratio(xd.grad.cpu(), *od.dgrad(dy, w), k)}
    ratios.update(_grad_ratios(wd.grad.reshape(d, k), bd.grad, x, dy, k))
    _report("autograd bf16", ratios)
