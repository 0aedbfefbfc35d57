"""GPU checks of the 3x3-convolution data gradient (csrc/convdgrad.hip, seld_native.conv3x3_dgrad) that
model_crnn._Conv3x3.backward uses for the encoder's blocks 2-4 in place of a weight flip / transpose launch and a
forward convolution of the library.

Reference: float64 conv2d(dy, flip-transposed w, padding=1) on the same bf16 values (CPU).  The bar per element is one
bf16 rounding of the result plus a worst-case fp32 accumulation over K = 9 * Cout terms in any order:

    |got - ref| <= 2^-8 |ref| + 2 * 9 * Cout * 2^-24 * S,      S = the same convolution of |dy| and |w|

No measured constant enters it.
"""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


def _inputs(b, t, f, cin, cout, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    dy = torch.randn(b, cout, t, f, generator=g).to(torch.bfloat16)
    w = (torch.randn(cout, cin, 3, 3, generator=g) * 0.05).to(torch.bfloat16)
    return dy, w


def _on_device(x, device):
    return x.to(device).contiguous(memory_format=torch.channels_last)


def _reference(dy, w):
    """float64 data gradient and the magnitude sum S of its terms (CPU tensors in, CPU float64 out)."""
    wt = w.double().transpose(0, 1).flip(2, 3)
    return F.conv2d(dy.double(), wt, padding=1), F.conv2d(dy.double().abs(), wt.abs(), padding=1)


def _worst(got, ref, mag, cout):
    bound = 2.0 ** -8 * ref.abs() + 2 * 9 * cout * 2.0 ** -24 * mag
    err = (got.double().cpu() - ref).abs()
    return (err / (bound + 1e-300)).max().item(), err.max().item()


# (B, T, F, Cin, Cout).  The first five are the smallest that exercise each index path: one partial chunk with nothing
# but halo rows above and below; two clips and two K chunks; every F; Cout = 64.  The kernel's position tile is 256
# (TC = 32 / 16 / 8 time rows at F = 8 / 16 / 32), so one full chunk plus one row for each F follows, and its N tile is
# 128 where Cin allows, so (1, 3, 8, 256, 128) runs two N tiles.
SHAPES = [(1, 1, 8, 64, 64), (2, 17, 8, 64, 128), (2, 9, 16, 128, 128), (2, 5, 32, 64, 128), (3, 16, 8, 128, 64),
          (1, 33, 8, 64, 64), (2, 17, 16, 128, 64), (1, 9, 32, 64, 64), (1, 3, 8, 256, 128)]


@pytest.mark.parametrize("b,t,f,cin,cout", SHAPES)
def test_matches_float64_convolution(gpu_device, b, t, f, cin, cout):
    import seld_native
    dy, w = _inputs(b, t, f, cin, cout, seed=1000 * b + 10 * t + f + cin + cout)
    ref, mag = _reference(dy, w)
    dyd, wd = _on_device(dy, gpu_device), _on_device(w, gpu_device)
    assert seld_native.conv3x3_dgrad_applicable(dyd, wd)
    dx = seld_native.conv3x3_dgrad(dyd, wd)
    torch.cuda.synchronize()
    assert dx.shape == (b, cin, t, f) and dx.dtype == torch.bfloat16
    assert dx.is_contiguous(memory_format=torch.channels_last)
    worst, err = _worst(dx, ref, mag, cout)
    print(f"\n{(b, t, f, cin, cout)}: worst error / bound {worst:.3f}, max abs error {err:.3e}")
    assert worst <= 1.0, (worst, err, ref.abs().max().item())


def test_nothing_crosses_a_clip_boundary(gpu_device):
    """dy is non-zero only in the last time row of clip 0: clip 1's dx is exactly zero (and clip 0's is right)."""
    import seld_native
    b, t, f, cin, cout = 2, 5, 8, 64, 64
    dy, w = _inputs(b, t, f, cin, cout, seed=11)
    dy[1] = 0
    dy[0, :, :t - 1] = 0
    dx = seld_native.conv3x3_dgrad(_on_device(dy, gpu_device), _on_device(w, gpu_device))
    torch.cuda.synchronize()
    assert torch.count_nonzero(dx[0]).item() > 0
    assert torch.count_nonzero(dx[1]).item() == 0
    ref, mag = _reference(dy, w)
    assert _worst(dx, ref, mag, cout)[0] <= 1.0


@pytest.mark.parametrize("f", [8, 16, 32])
@pytest.mark.parametrize("edge", ["last", "first"])
def test_nothing_wraps_round_a_frequency_edge(gpu_device, f, edge):
    """dy is non-zero only in the last (first) frequency column: dx is exactly zero beyond the neighbouring column, in
    particular in the first (last) column of the next (previous) time row, where a wrap-around would land."""
    import seld_native
    b, t, cin, cout = 2, 4, 64, 64
    dy, w = _inputs(b, t, f, cin, cout, seed=12 + f)
    keep = f - 1 if edge == "last" else 0
    mask = torch.zeros(f, dtype=torch.bool)
    mask[keep] = True
    dy[..., ~mask] = 0
    dx = seld_native.conv3x3_dgrad(_on_device(dy, gpu_device), _on_device(w, gpu_device))
    torch.cuda.synchronize()
    far = dx[..., :f - 2] if edge == "last" else dx[..., 2:]
    near = dx[..., f - 2:] if edge == "last" else dx[..., :2]
    assert torch.count_nonzero(far).item() == 0
    assert torch.count_nonzero(near).item() > 0
    ref, mag = _reference(dy, w)
    assert _worst(dx, ref, mag, cout)[0] <= 1.0


@pytest.mark.parametrize("b,t,f,cin,cout", [(2, 17, 8, 64, 64), (1, 9, 32, 64, 64), (2, 3, 16, 256, 64)])
def test_writes_nothing_outside_dx(gpu_device, b, t, f, cin, cout):
    """dx is a slice of a larger buffer of a sentinel pattern with guard rows before and after (T is not a multiple
    of the time rows per chunk: the ragged last chunk of every clip): the guards come back bit-identical."""
    import seld_native
    dy, w = _inputs(b, t, f, cin, cout, seed=13)
    guard, n = 64 * cin, b * t * f * cin
    pattern = (torch.arange(n + 2 * guard, dtype=torch.int32) % 251 + 0x3F00).to(torch.int16).to(gpu_device)
    buf = pattern.clone()
    out = buf[guard:guard + n].view(torch.bfloat16).view(b, t, f, cin).permute(0, 3, 1, 2)
    dx = seld_native.conv3x3_dgrad(_on_device(dy, gpu_device), _on_device(w, gpu_device), out=out)
    torch.cuda.synchronize()
    assert dx.data_ptr() == out.data_ptr()
    assert torch.equal(buf[:guard], pattern[:guard])
    assert torch.equal(buf[guard + n:], pattern[guard + n:])
    ref, mag = _reference(dy, w)
    assert _worst(dx, ref, mag, cout)[0] <= 1.0


def test_two_calls_are_bit_identical(gpu_device):
    import seld_native
    dy, w = _inputs(3, 40, 16, 128, 128, seed=14)
    dyd, wd = _on_device(dy, gpu_device), _on_device(w, gpu_device)
    a = seld_native.conv3x3_dgrad(dyd, wd)
    b = seld_native.conv3x3_dgrad(dyd, wd)
    torch.cuda.synchronize()
    assert torch.equal(a, b)


@pytest.mark.parametrize("f,cin,cout", [(64, 64, 64), (8, 4, 64), (8, 96, 64), (8, 64, 32), (16, 64, 96)])
def test_unsupported_shapes_are_refused(gpu_device, f, cin, cout):
    import seld_native
    dy, w = _inputs(1, 2, f, cin, cout, seed=15)
    dyd, wd = _on_device(dy, gpu_device), _on_device(w, gpu_device)
    assert not seld_native.conv3x3_dgrad_applicable(dyd, wd)
    with pytest.raises(seld_native.SeldNativeError):
        seld_native.conv3x3_dgrad(dyd, wd)
    seld_native.ensure_init(gpu_device)
    dx = torch.empty(1, cin, 2, f, dtype=torch.bfloat16, device=gpu_device).contiguous(memory_format=torch.channels_last)
    lib = seld_native.load_library()
    rc = lib.seld_conv3x3_dgrad(dyd.data_ptr(), wd.data_ptr(), 1, 2, f, cin, cout, dx.data_ptr(), None)
    assert rc == -4, rc                                                   # kErrUnsupported (include/seld_hip.h)


def test_conv_block_backward_with_and_without_the_kernel(gpu_device):
    """One ConvBlock(64, 128) under bf16 autocast at (B, T, F) = (2, 9, 32), the same graph differentiated with
    FUSED_CONV_DGRAD on and off: the input gradients stay within the parity bound of each other, the weight gradient
    (its inputs did not change) is bit-identical, and the block that uses the kernel launches no weight transform."""
    import model_crnn
    import seld_native
    torch.manual_seed(3)
    block = model_crnn.ConvBlock(64, 128, pool_size=(1, 2)).to(gpu_device).to(memory_format=torch.channels_last).train()
    x = torch.randn(2, 64, 9, 32, device=gpu_device).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    x.requires_grad_(True)
    with torch.autocast(device_type="cuda", dtype=torch.bfloat16):
        y = block(x)
    gy = torch.randn(y.shape, device=gpu_device).to(y.dtype).contiguous(memory_format=torch.channels_last)

    flips, seen = [], []
    real_flip, real_dgrad = seld_native.conv_weight_flip_transpose, seld_native.conv3x3_dgrad

    def counted_flip(w):
        flips.append(tuple(w.shape))
        return real_flip(w)

    def recording_dgrad(dy, w, out=None):
        seen.append((dy.detach().clone(), w.detach().clone()))
        return real_dgrad(dy, w, out)

    was = model_crnn._Conv3x3.fused_dgrad
    grads = {}
    try:
        seld_native.conv_weight_flip_transpose = counted_flip
        seld_native.conv3x3_dgrad = recording_dgrad
        for on in (True, False):
            model_crnn._Conv3x3.fused_dgrad = on
            flips.clear()
            grads[on] = torch.autograd.grad(y, (x, block.conv.weight), gy, retain_graph=True)
            torch.cuda.synchronize()
            assert (len(flips) == 0) if on else (len(flips) == 1), (on, flips)
    finally:
        seld_native.conv_weight_flip_transpose = real_flip
        seld_native.conv3x3_dgrad = real_dgrad
        model_crnn._Conv3x3.fused_dgrad = was
    assert len(seen) == 1                                                 # the kernel ran once, for the "on" pass
    dy, w = seen[0]
    ref, mag = _reference(dy.cpu(), w.cpu())
    bound = 2.0 ** -8 * ref.abs() + 2 * 9 * 128 * 2.0 ** -24 * mag
    assert ((grads[True][0].double().cpu() - ref).abs() <= bound).all()   # the kernel against the float64 reference
    # the library's result is one rounding and one accumulation away from the reference as well
    assert ((grads[True][0].double() - grads[False][0].double()).abs().cpu() <= 2 * bound).all()
    assert torch.equal(grads[True][1], grads[False][1])
