"""GPU tests of the chunk pipeline and the 2 x 4 wave grid of the 3x3-convolution weight-gradient kernel
(csrc/convwgrad.hip, seld_native.conv3x3_wgrad): one 8-wave workgroup per CU that computes on one LDS image while the
next chunk waits in registers and is then stored into the other image.

Reference and bound are those of tests/test_conv_wgrad_gpu.py (restated here): aten.convolution_backward in fp32 on the
same bf16-rounded inputs; both sides accumulate in fp32 in different orders, so the bar is an fp32 accumulation error --
1e-5 times the sum of |terms|, computed as the same product of |dy| and |x| -- plus, for a bf16 gradient, one bf16
rounding (2^-8 relative).

The cases are the smallest that reach each state of the pipeline on a 256-CU device; the slab count each is meant to
reach is asserted from the reported workspace size, so that a later change of the plan cannot silently turn them into
one-chunk cases.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

# (b, cin, cout, t, f), K slabs the plan must give on 256 CUs, chunks per slab
CASES = [((3, 64, 64, 37, 8), 9, 1),          # prologue = epilogue; ragged last time rows (37 = 2 * 16 + 5)
         ((4, 128, 128, 250, 16), 64, 2),     # both images used once
         ((2, 128, 256, 190, 32), 32, 3),     # T not a multiple of the 4 time rows per chunk; steady state
         ((3, 256, 256, 270, 8), 13, 4),      # 51 chunks: the last slab holds 3
         ((1, 64, 192, 3, 32), None, None)]   # a clip shorter than one chunk
FOUR_CHUNKS = CASES[3][0]


def _case(b, cin, cout, t, f, device, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    x = torch.randn(b, cin, t, f, generator=g).to(device=device, dtype=torch.bfloat16)
    dy = (torch.randn(b, cout, t, f, generator=g) * 0.1).to(device=device, dtype=torch.bfloat16)
    cl = torch.channels_last
    return x.contiguous(memory_format=cl), dy.contiguous(memory_format=cl)


def _reference(x, dy, cin):
    w = torch.empty(dy.shape[1], cin, 3, 3, device=x.device)
    args = ((1, 1), (1, 1), (1, 1), False, (0, 0), 1, (False, True, False))
    ref = torch.ops.aten.convolution_backward(dy.float(), x.float(), w, None, *args)[1]
    mag = torch.ops.aten.convolution_backward(dy.float().abs(), x.float().abs(), w, None, *args)[1]
    return ref, mag


def _dw(cout, cin, dtype, device):
    return torch.empty(cout, cin, 3, 3, dtype=dtype, device=device, memory_format=torch.channels_last)


def _slabs(b, cin, cout, t, f, device):
    import seld_native
    seld_native.ensure_init(device)
    floats = seld_native.load_library().seld_conv3x3_wgrad_workspace_floats(b, t, f, cin, cout)
    assert floats > 0 and floats % (cout * 9 * cin) == 0, floats
    return floats // (cout * 9 * cin)


@pytest.mark.parametrize("shape,slabs,per_slab", CASES)
def test_pipeline_states_match_convolution_backward(gpu_device, shape, slabs, per_slab):
    import seld_native
    b, cin, cout, t, f = shape
    if slabs is not None:
        chunks = b * -(-t // (128 // f))
        got = _slabs(b, cin, cout, t, f, gpu_device)
        assert got == slabs and -(-chunks // got) == per_slab, (shape, chunks, got)
    x, dy = _case(b, cin, cout, t, f, gpu_device, seed=b * 1000 + cin + f)
    assert seld_native.conv3x3_wgrad_applicable(x, dy, _dw(cout, cin, torch.bfloat16, gpu_device))
    ref, mag = _reference(x, dy, cin)
    for dtype, rounding in ((torch.float32, 0.0), (torch.bfloat16, 2.0 ** -8)):
        dw = seld_native.conv3x3_wgrad(x, dy, _dw(cout, cin, dtype, gpu_device))
        torch.cuda.synchronize()
        err = (dw.float() - ref).abs()
        bound = 1e-5 * mag + rounding * ref.abs() + 1e-30
        worst = (err / bound).max().item()
        print(f"\n{shape} {dtype}: worst err / bound = {worst:.3f}, max |err| = {err.max().item():.3e}")
        assert worst <= 1.0, (dtype, worst, err.max().item(), ref.abs().max().item())


def test_two_calls_are_bit_identical_over_four_chunks(gpu_device):
    import seld_native
    b, cin, cout, t, f = FOUR_CHUNKS
    x, dy = _case(b, cin, cout, t, f, gpu_device, seed=7)
    for dtype in (torch.bfloat16, torch.float32):
        first = seld_native.conv3x3_wgrad(x, dy, _dw(cout, cin, dtype, gpu_device))
        second = seld_native.conv3x3_wgrad(x, dy, _dw(cout, cin, dtype, gpu_device))
        torch.cuda.synchronize()
        assert torch.equal(first, second), dtype


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_nothing_outside_dw_is_written(gpu_device, dtype):
    import seld_native
    b, cin, cout, t, f = CASES[0][0]
    x, dy = _case(b, cin, cout, t, f, gpu_device, seed=11)
    n, pad, sentinel = cout * 9 * cin, 64, -7.0                # 64 elements keep dw 16-byte aligned in both dtypes
    buf = torch.full((n + 2 * pad,), sentinel, dtype=dtype, device=gpu_device)
    dw = buf[pad:pad + n].view(cout, 3, 3, cin).permute(0, 3, 1, 2)      # [Cout, Cin, 3, 3] in channels-last memory
    seld_native.conv3x3_wgrad(x, dy, dw)
    torch.cuda.synchronize()
    assert (buf[:pad] == sentinel).all() and (buf[pad + n:] == sentinel).all()
    assert torch.equal(dw, seld_native.conv3x3_wgrad(x, dy, _dw(cout, cin, dtype, gpu_device)))


def test_bench_shapes_use_one_workgroup_per_cu_of_workspace(gpu_device):
    for b, cin, cout, t, f in ((32, 64, 128, 250, 32), (32, 128, 256, 250, 16), (32, 256, 512, 250, 8)):
        slabs = _slabs(b, cin, cout, t, f, gpu_device)
        assert slabs * cout * 9 * cin <= 256 * 64 * 9 * 64, (cin, cout, slabs)
