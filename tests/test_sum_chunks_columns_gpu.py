"""GPU tests of the chunk sum that writes its columns in (channel, frequency) order (csrc/glue.hip
sum_chunks_columns_kernel, seld_native.sum_chunks(..., columns_cf=(C, F))): dW_ih of the first GRU layer leaves the
split-K reduction in the parameter's own column order instead of going through a strided copy.

The mapped sum accumulates every element exactly as the plain one does (fp32, chunks in order, one rounding), so the
bar is bit equality with ``sum_chunks`` followed by the framework's permute."""
import pytest
import torch

pytestmark = pytest.mark.gpu

ROWS = 5


@pytest.mark.parametrize("chunks", [1, 3, 8, 9])
@pytest.mark.parametrize("c,f", [(8, 4), (512, 4), (64, 2), (24, 3)])
@pytest.mark.parametrize("in_dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("out_dtype", [torch.bfloat16, torch.float32])
def test_equals_sum_then_permute(gpu_device, chunks, c, f, in_dtype, out_dtype):
    import seld_native
    g = torch.Generator().manual_seed(chunks * 10000 + c * 10 + f)
    partial = torch.randn(chunks, ROWS, f * c, generator=g).to(device=gpu_device, dtype=in_dtype)
    plain = seld_native.sum_chunks(partial, torch.empty(ROWS, f * c, dtype=out_dtype, device=gpu_device))
    want = plain.view(ROWS, f, c).transpose(1, 2).reshape(ROWS, c * f)
    n, pad, sentinel = ROWS * c * f, 64, -3.0                  # 64 elements keep ``out`` 16-byte aligned in both dtypes
    buf = torch.full((n + 2 * pad,), sentinel, dtype=out_dtype, device=gpu_device)
    out = buf[pad:pad + n].view(ROWS, c * f)
    assert seld_native.sum_chunks(partial, out, columns_cf=(c, f)) is out
    torch.cuda.synchronize()
    assert torch.equal(out, want)
    assert (buf[:pad] == sentinel).all() and (buf[pad + n:] == sentinel).all()


def test_tall_product_writes_the_permuted_columns(gpu_device):
    from seld_linear import chunk_count, tall_product
    c, f, n, rows = 16, 4, 2048, 24
    assert chunk_count(n, rows, c * f) > 1
    g = torch.Generator().manual_seed(3)
    a = torch.randn(n, rows, generator=g).to(device=gpu_device, dtype=torch.bfloat16)
    x = torch.randn(n, f * c, generator=g).to(device=gpu_device, dtype=torch.bfloat16)
    for dtype in (torch.bfloat16, torch.float32):
        want = tall_product(a, x, out_dtype=dtype).view(rows, f, c).transpose(1, 2).reshape(rows, c * f)
        out = torch.empty(rows, c * f, dtype=dtype, device=gpu_device)
        assert tall_product(a, x, out=out, columns_cf=(c, f)) is out
        assert torch.equal(out, want)


# B = 2, T = 6: 12 rows, which tall_product multiplies as one GEMM and permutes with a framework copy;
# B = 4, T = 256: 1024 rows = 4 chunks, the split-K product that ends in sum_chunks_columns_kernel (the training path)
@pytest.mark.parametrize("b,t,chunks", [(2, 6, 1), (4, 256, 4)])
def test_bigru_layer_dw_ih_equals_the_channel_major_layer(gpu_device, b, t, chunks):
    """_BiGRULayer with feature_cf = (512, 4) on (frequency, channel)-ordered features against the same layer fed the
    (channel, frequency)-ordered features with feature_cf = None: the two products multiply the same numbers in the same
    order (a column permutation of both GEMM operands), so dW_ih has to agree bit for bit.  The input projection of the
    forward pass sums over the permuted axis, so its inputs are small integers (x) and multiples of 2^-7 (W_ih): every
    partial sum is then exact in fp32 and the projection does not depend on the order either."""
    import seld_gru
    from seld_linear import chunk_count
    c, f, h = 512, 4, seld_gru.HIDDEN
    assert chunk_count(b * t, 6 * h, c * f) == chunks
    g = torch.Generator().manual_seed(17)
    x_cf = torch.randint(-3, 4, (b, t, c, f), generator=g).float().to(gpu_device)        # features ordered c * F + f
    w_ih = (torch.randint(-4, 5, (6 * h, c * f), generator=g).float() / 128).to(gpu_device)
    b_ih = (torch.randn(6 * h, generator=g) * 0.1).to(gpu_device)
    w_hh = (torch.randn(2, 3 * h, h, generator=g) * 0.05).to(gpu_device)
    b_hh = (torch.randn(2, 3 * h, generator=g) * 0.1).to(gpu_device)
    dy = torch.randn(b, t, 2 * h, generator=g).to(device=gpu_device, dtype=torch.bfloat16)

    def dw_ih(x, feature_cf):
        w = w_ih.clone().requires_grad_(True)
        x = x.clone().requires_grad_(True)                     # as in the model: the features come from the encoder
        with torch.autocast(device_type="cuda", dtype=torch.bfloat16):
            y = seld_gru._BiGRULayer.apply(x, w, b_ih, w_hh, b_hh, False, feature_cf)
        y.backward(dy.to(y.dtype))
        torch.cuda.synchronize()
        return w.grad

    plain = dw_ih(x_cf.reshape(b, t, c * f), None)
    mapped = dw_ih(x_cf.transpose(2, 3).reshape(b, t, f * c), (c, f))
    assert plain.abs().max().item() > 0
    assert torch.equal(mapped, plain)
