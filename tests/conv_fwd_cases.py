"""Inputs and float64 references shared by tests/test_conv_fwd_cpu.py and tests/test_conv_fwd_gpu.py (csrc/convfwd.hip).
Every reference is computed once per process and handed out as is: the tests do not modify what they get."""
import functools

import torch
import torch.nn.functional as F

# (B, T, F, Cin, Cout), the smallest that reach each index path of the kernel (position tile 256 = 32 / 16 / 8 time rows
# at F = 8 / 16 / 32; result tile 128 channels where Cout allows, else 64; K slices of 64 input channels):
SHAPES = [(1, 1, 8, 64, 64),        # one ragged chunk; the 64-wide tile
          (2, 33, 8, 64, 128),      # a full chunk plus one row; two clips; the 128-wide tile
          (2, 17, 16, 128, 128),    # two K slices; ragged chunk at F = 16
          (2, 9, 32, 64, 128),      # block 2's class; ragged chunk at F = 32
          (1, 3, 8, 128, 256),      # two N tiles
          (1, 5, 16, 64, 192)]      # three 64-wide tiles

BLOCK_SHAPE = (2, 9, 32, 64, 128)   # ConvBlock(64, 128) at (B, T, F) = (2, 9, 32)


def chunks(b, t, f):
    tc = 256 // f
    return b * ((t + tc - 1) // tc)


@functools.lru_cache(maxsize=None)
def inputs(b, t, f, cin, cout, seed=None):
    g = torch.Generator(device="cpu").manual_seed(1000 * b + 10 * t + f + cin + cout if seed is None else seed)
    x = torch.randn(b, cin, t, f, generator=g).to(torch.bfloat16)
    w = (torch.randn(cout, cin, 3, 3, generator=g) * 0.05).to(torch.bfloat16)
    return x, w


def reference(x, w):
    """float64 convolution of the bf16 values and the magnitude sum S of its terms."""
    return F.conv2d(x.double(), w.double(), padding=1), F.conv2d(x.double().abs(), w.double().abs(), padding=1)


@functools.lru_cache(maxsize=None)
def case(b, t, f, cin, cout):
    x, w = inputs(b, t, f, cin, cout)
    return (x, w) + reference(x, w)


def bound(ref, mag, cin):
    """One bf16 rounding of the result plus a worst-case fp32 accumulation over K = 9 * Cin terms in any order."""
    return 2.0 ** -8 * ref.abs() + 2 * 9 * cin * 2.0 ** -24 * mag


@functools.lru_cache(maxsize=None)
def integer_case():
    """x in {-1, 0, 1}, w in {-1, 0, 1} with exactly 128 non-zeros per output channel, at the ragged BLOCK_SHAPE: the
    convolution is integer-valued with |y| <= 128."""
    b, t, f, cin, cout = BLOCK_SHAPE
    g = torch.Generator(device="cpu").manual_seed(77)
    x = torch.randint(-1, 2, (b, cin, t, f), generator=g).to(torch.bfloat16)
    w = torch.zeros(cout, cin * 9)
    for co in range(cout):
        idx = torch.randperm(cin * 9, generator=g)[:128]
        w[co, idx] = (torch.randint(0, 2, (128,), generator=g) * 2 - 1).float()
    w = w.view(cout, cin, 3, 3).to(torch.bfloat16)
    return x, w, F.conv2d(x.double(), w.double(), padding=1)


@functools.lru_cache(maxsize=None)
def block_case():
    """ConvBlock(64, 128) with pooling at BLOCK_SHAPE: parameters, input, and the float64 forward of the bf16 values:
    conv output y, its bound, the BatchNorm coefficients a, b (z = a y + b) per channel."""
    b, t, f, cin, cout = BLOCK_SHAPE
    g = torch.Generator(device="cpu").manual_seed(5)
    x = torch.randn(b, cin, t, f, generator=g).to(torch.bfloat16)
    w = torch.randn(cout, cin, 3, 3, generator=g) * (2.0 / (9 * cin)) ** 0.5
    gamma = torch.rand(cout, generator=g) + 0.5
    beta = torch.randn(cout, generator=g) * 0.5
    y, mag = reference(x, w.to(torch.bfloat16))
    mean = y.mean((0, 2, 3))
    var = y.var((0, 2, 3), unbiased=False)
    a = gamma.double() / torch.sqrt(var + 1e-5)
    bb = beta.double() - mean * a
    return {"x": x, "w": w, "gamma": gamma, "beta": beta, "y": y, "bound": bound(y, mag, cin), "a": a, "b": bb}


def block_safe_mask(c):
    """Pooled output elements of ``block_case`` whose ReLU and pooling decisions cannot change when every conv output
    moves by up to twice its bound: both pre-activations z = a y + b of the pair are farther than m = |a| * 2 * bound
    from zero and from each other (m of the pair summed for the comparison of the two)."""
    z = c["a"].view(1, -1, 1, 1) * c["y"] + c["b"].view(1, -1, 1, 1)
    m = c["a"].abs().view(1, -1, 1, 1) * 2 * c["bound"]
    z0, z1, m0, m1 = z[..., 0::2], z[..., 1::2], m[..., 0::2], m[..., 1::2]
    return (z0.abs() > m0) & (z1.abs() > m1) & ((z0 - z1).abs() > m0 + m1)
