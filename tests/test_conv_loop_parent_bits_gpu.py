"""GPU checks that the main loop of csrc/conv3x3_loop.h, whose loads and LDS reads were moved under the MFMAs and whose
epilogue now stores 16 bytes per lane after a swap between lane rows, still adds every product to its accumulator in
the same order and writes every value where it belongs: the forward outputs with their ``partials`` rows
(csrc/convfwd.hip) and the data gradients (csrc/convdgrad.hip) are compared bit for bit with what the build of the
commit before that change wrote for the same seeded inputs, tests/golden/conv3x3_loop_parent.npz (recorded by
tools/record_conv_loop_fixture.py; bf16 / fp32 bit patterns).

Shapes (B, T, F, Cin, Cout), the smallest that reach each path of the loop (a stage = one tap x 64 K channels; the
weight slice of stage s + 1 is requested during stage s, the last stage requests its own slice again):
  (1, 1, 8, 64, 64)       one ragged chunk, nine stages, the 64-wide result tile            forward, data gradient
  (2, 33, 8, 128, 128)    two K slices, two chunks per clip, the 128-wide tile              forward
  (2, 17, 16, 192, 128)   three K slices, ragged at F = 16                                  forward
  (2, 9, 32, 64, 128)     block 2's class                                                   forward, data gradient
  (2, 9, 32, 128, 64)     block 2's class with the channel counts as the gradient sees them data gradient
  (1, 3, 8, 256, 128)     two result tiles                                                  data gradient
  (1, 3, 8, 128, 256)     four K slices                                                     data gradient
Two further checks run at (2, 33, 8, 128, 128) and (2, 17, 16, 192, 128) in both directions, sizes at which several
K slices meet a ragged chunk: two calls give the same bits, and nothing is written outside the result."""
import functools
from pathlib import Path

import numpy as np
import pytest
import torch

import conv_fwd_cases as cases

pytestmark = pytest.mark.gpu

FIXTURE = Path(__file__).resolve().parent / "golden" / "conv3x3_loop_parent.npz"
FWD = [(1, 1, 8, 64, 64), (2, 33, 8, 128, 128), (2, 17, 16, 192, 128), (2, 9, 32, 64, 128)]
DGRAD = [(1, 1, 8, 64, 64), (2, 9, 32, 128, 64), (2, 9, 32, 64, 128), (1, 3, 8, 256, 128), (1, 3, 8, 128, 256)]
BOTH = [(2, 33, 8, 128, 128), (2, 17, 16, 192, 128)]


def key(direction, shape, what):
    return f"{direction}_{'_'.join(map(str, shape))}_{what}"


def fwd_inputs(shape):
    return cases.inputs(*shape)


@functools.lru_cache(maxsize=None)
def dgrad_inputs(shape):
    b, t, f, cin, cout = shape
    g = torch.Generator(device="cpu").manual_seed(7000 + 1000 * b + 10 * t + f + cin + 3 * cout)
    dy = torch.randn(b, cout, t, f, generator=g).to(torch.bfloat16)
    w = (torch.randn(cout, cin, 3, 3, generator=g) * 0.05).to(torch.bfloat16)
    return dy, w


def on_device(x, device):
    return x.to(device).contiguous(memory_format=torch.channels_last)


def bits(x):
    """Bit patterns of a device tensor as a numpy array (bf16 in channels-last order -> int16, fp32 -> int32)."""
    if x.dtype == torch.bfloat16:
        return x.permute(0, 2, 3, 1).contiguous().view(torch.int16).cpu().numpy()
    return x.contiguous().view(torch.int32).cpu().numpy()


def run_forward(seld_native, shape, device):
    x, w = fwd_inputs(shape)
    xd, wd = on_device(x, device), on_device(w, device)
    plain = seld_native.conv3x3_forward(xd, wd)
    y, partials = seld_native.conv3x3_forward(xd, wd, stats=True)
    torch.cuda.synchronize()
    return plain, y, partials


def run_dgrad(seld_native, shape, device):
    dy, w = dgrad_inputs(shape)
    dx = seld_native.conv3x3_dgrad(on_device(dy, device), on_device(w, device))
    torch.cuda.synchronize()
    return dx


@functools.lru_cache(maxsize=None)
def fixture():
    return dict(np.load(FIXTURE))


@pytest.mark.parametrize("shape", FWD)
def test_forward_and_partials_have_the_parent_bits(gpu_device, shape):
    import seld_native
    plain, y, partials = run_forward(seld_native, shape, gpu_device)
    want = fixture()
    assert np.array_equal(bits(y), want[key("fwd", shape, "y")])
    assert np.array_equal(bits(plain), want[key("fwd", shape, "y")])          # the instantiation without the sums
    assert np.array_equal(bits(partials), want[key("fwd", shape, "partials")])


@pytest.mark.parametrize("shape", DGRAD)
def test_data_gradient_has_the_parent_bits(gpu_device, shape):
    import seld_native
    dx = run_dgrad(seld_native, shape, gpu_device)
    assert np.array_equal(bits(dx), fixture()[key("dgrad", shape, "dx")])


def _guarded(shape_nhwc, device):
    """A sentinel buffer with guard rows before and after a bf16 [B, C, T, F] channels-last view of its middle."""
    b, t, f, c = shape_nhwc
    guard, n = 64 * c, b * t * f * c
    pattern = (torch.arange(n + 2 * guard, dtype=torch.int32) % 251 + 0x3F00).to(torch.int16).to(device)
    buf = pattern.clone()
    out = buf[guard:guard + n].view(torch.bfloat16).view(b, t, f, c).permute(0, 3, 1, 2)
    return pattern, buf, out, guard, n


@pytest.mark.parametrize("shape", BOTH)
def test_forward_twice_the_same_bits_and_nothing_outside_the_result(gpu_device, shape):
    import seld_native
    b, t, f, cin, cout = shape
    x, w = fwd_inputs(shape)
    xd, wd = on_device(x, gpu_device), on_device(w, gpu_device)
    first, first_partials = seld_native.conv3x3_forward(xd, wd, stats=True)
    pattern, buf, out, guard, n = _guarded((b, t, f, cout), gpu_device)
    rows = cases.chunks(b, t, f)
    fill = torch.full(((rows + 4) * 2 * cout,), -7.0, device=gpu_device)
    partials = fill[4 * cout:4 * cout + 2 * rows * cout].view(2, rows, cout)
    y, p = seld_native.conv3x3_forward(xd, wd, stats=True, out=out, partials=partials)
    torch.cuda.synchronize()
    assert y.data_ptr() == out.data_ptr() and p.data_ptr() == partials.data_ptr()
    assert torch.equal(buf[:guard], pattern[:guard]) and torch.equal(buf[guard + n:], pattern[guard + n:])
    assert (fill[:4 * cout] == -7.0).all() and (fill[4 * cout + 2 * rows * cout:] == -7.0).all()
    assert torch.equal(y, first) and torch.equal(p, first_partials)


@pytest.mark.parametrize("shape", BOTH)
def test_data_gradient_twice_the_same_bits_and_nothing_outside_the_result(gpu_device, shape):
    import seld_native
    b, t, f, cin, cout = shape
    dy, w = dgrad_inputs(shape)
    dyd, wd = on_device(dy, gpu_device), on_device(w, gpu_device)
    first = seld_native.conv3x3_dgrad(dyd, wd)
    pattern, buf, out, guard, n = _guarded((b, t, f, cin), gpu_device)
    dx = seld_native.conv3x3_dgrad(dyd, wd, out=out)
    torch.cuda.synchronize()
    assert dx.data_ptr() == out.data_ptr()
    assert torch.equal(buf[:guard], pattern[:guard]) and torch.equal(buf[guard + n:], pattern[guard + n:])
    assert torch.equal(dx, first)
