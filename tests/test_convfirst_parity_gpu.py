"""Element-wise parity of the first encoder block's kernels (csrc/convfirst.hip) with an exact float64 replay, on the
card: every F the kernels accept, partial and ragged chunks, single rows, the grid-stride chunk walk, clip and frequency
edges, every weight path and every dw target, guard regions, ``phases``, repeatability and the refusals.

The kernels never store the convolution output, so the inputs are chosen such that it is known to the bit
(tests/convfirst_checks.py: an integer and a dyadic family whose fp32 accumulation is exact in any order).  Then y and
dbeta are compared bit for bit, a / b / mean with the fp32 expressions of the kernel's own returned values, and every
element of dW with the float64 weight gradient under a derived bound (the checks' docstrings state each one).  Every
test prints the error / bound ratio of every check; all must be <= 1.

Measured on an MI355X, 256 compute units (worst error / bound per check, as the tests print them; "int" / "dy" = the
integer / dyadic family).  finite, a, b, y, dbeta and the integer family's mean are 0 (bit-equal) everywhere.

  test                     invstd       running_mean  running_var  mean (dy)  var (dy)  dgamma int / dy   dw.ambiguous  dw
  small shapes, bf16 dw    0.50 / 0.63  0.50          0.50 / 0.52  2.2e-3     0.032     0.50 / 7.5e-3     0.78          0.99
    per shape, dw:         (2,3,16) 0.98  (2,11,32) 0.97  (3,5,64) 0.96  (2,3,128) 0.98  (2,3,256) 0.99  (1,1,16) 0.98
                           (1,1,256) 0.94  (3,17,16) 0.95
    per shape, invstd dy:  0.56  0.60  0.53  0.63  0.55  0.50  0.55  0.57  (same order)
  momentum 0.25, fp32 dw   0.50 / 0.58  0.50          0.49 / 0.50  1.1e-3     0.030     0.49 / 1.0e-3     0.30          4.6e-3
  walk (5,211,256)         0.50 / 0.56  0.50          0.50 / 0.50  2.5e-5     0.011     0.50 / 4.0e-5     0.18          0.72
  walk (5,821,64), fp32 dw 0.49 / 0.60  0.50          0.50 / 0.51  1.8e-5     0.0094    0.49 / 4.9e-5     0.22          3.2e-4
  edges                    0.50 / 0.50  0.50          0.50 / 0.50  8.7e-3     0.027     0.50 / 9.1e-3     0.094         0.995
  weight paths, phases     0.50 / 0.64  0.50          0.49 / 0.51  5.0e-4     0.029     0.49 / 1.9e-3     0.58          0.97

A bf16 dw sits just under 1 wherever an element's rounding error nears half an ulp just above a power of two: that is
the 2^-8 |ref| store term, which the check cannot tighten without knowing the fp32 sum.  The fp32 rows show the
accumulation itself: under 1 % of D_w u S.

One check failed when these tests first ran and was fixed in csrc/convfirst.hip: invstd of the dyadic family at
(1, 1, 256), 1.09 fp32 ulp before, 0.55 after (test_every_element_on_the_small_shapes has the account).
"""
import pytest
import torch

import convfirst_checks as cc

pytestmark = pytest.mark.gpu

CL = torch.channels_last
BF16 = torch.bfloat16
INVALID, UNSUPPORTED = -1, -4           # SELD_ERR_INVALID_ARGUMENT, SELD_ERR_UNSUPPORTED (include/seld_hip.h)
FAMILIES = ["integer", "dyadic"]

# (B, T, F); 256 / F time rows per chunk: 16, 8, 4, 2, 1
SHAPES = [(2, 3, 16),        # T < rows per chunk: both clips are partial chunks
          (2, 11, 32),       # ragged second chunk
          (3, 5, 64),        # ragged second chunk
          (2, 3, 128),       # ragged second chunk
          (2, 3, 256),       # 3 chunks per clip
          (1, 1, 16),        # a single row with padding above and below
          (1, 1, 256),
          (3, 17, 16)]       # one full chunk + 1 row


def _cus(device):
    return torch.cuda.get_device_properties(device).multi_processor_count


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF16 else torch.int32)


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


def _run(case, device, w=None, dw=None, phases=3):
    """One forward and backward through seld_native -> the kernels' outputs as CPU tensors (y as [rows / 2, 64]).
    w / dw: device tensors to use in place of the bf16 channels-last weight / a bf16 channels-last gradient."""
    import seld_native
    x = case["x"].to(device).contiguous(memory_format=CL)
    dy = case["dy"].to(device).contiguous(memory_format=CL)
    if w is None:
        w = case["w"].to(device).contiguous(memory_format=CL)
    if dw is None:
        dw = torch.empty(64, 4, 3, 3, dtype=BF16, device=device).contiguous(memory_format=CL)
    rm, rv = case["rm0"].to(device), case["rv0"].to(device)
    y, mi, ss = seld_native.convfirst_forward(x, w, case["weight"].to(device), case["bias"].to(device), rm, rv,
                                              case["momentum"], case["eps"], phases=phases)
    dw, dgamma, dbeta = seld_native.convfirst_backward(x, w, dy, mi, ss, dw, phases=phases)
    torch.cuda.synchronize()
    assert y.dtype == BF16 and y.is_contiguous(memory_format=CL)
    return dict(y=cc.rows_of(y).cpu(), mean_invstd=mi.cpu(), scale_shift=ss.cpu(), running_mean=rm.cpu(),
                running_var=rv.cpu(), dw=dw.cpu().contiguous(), dgamma=dgamma.cpu(), dbeta=dbeta.cpu())


def _report(what, ratios):
    print(f"\n{what}: {cc.fmt(ratios)}")
    assert cc.passes(ratios), cc.fmt(ratios)
    assert ratios["y"] == 0.0 and ratios["dbeta"] == 0.0


def _all_same(a, b):
    for k, v in a.items():
        assert _same(v, b[k]), k


# ------------------------------------------------------------------------------------------------- shapes

@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_every_element_on_the_small_shapes(gpu_device, shape, family):
    """(1, 1, 256) dyadic failed on invstd when this test first ran: 1.09 fp32 ulp from the float64 1 / sqrt(var + eps)
    against the bound of 1.  convfirst_stats_kernel chained its X^T X matrix products through one fp32 accumulator, and
    in the dyadic family the sums of squares are not exact (multiples of 2^-20 reaching 2^13 per wave); with one chunk
    there are only four fp32 partials and nothing for the double combination to average, so a relative error of 1.4 u
    in the variance came on top of the half ulp of invstd's own rounding.  The kernel now starts every matrix product
    from a zero accumulator and adds the results in double, through the waves and the partial rows (a float pair):
    0.55 ulp on this case, and the worst dyadic invstd of the file went from 1.09 to 0.64."""
    case = cc.make_case(family, shape)
    geom = cc.geometry(shape, _cus(gpu_device))
    assert geom["per_group"] == 1
    _report(f"{family} {shape}", cc.run_checks(case, _run(case, gpu_device), _cus(gpu_device)))


@pytest.mark.parametrize("family", FAMILIES)
def test_momentum_a_quarter_and_an_fp32_gradient(gpu_device, family):
    case = cc.make_case(family, (3, 5, 64), seed=1, momentum=0.25)
    dw = torch.empty(64, 4, 3, 3, dtype=torch.float32, device=gpu_device)
    _report(f"{family} momentum 0.25, fp32 dw", cc.run_checks(case, _run(case, gpu_device, dw=dw), _cus(gpu_device)))


def _walk_shape(f, cus):
    """(B, T, F) with 2 groups < chunks < 3 groups, groups = min(2 CUs, 512): every workgroup walks 2 or 3 chunks.
    256 compute units: (5, 211, 256) = 1055 chunks, (5, 821, 64) = 1030 chunks with a ragged last chunk per clip."""
    groups = min(2 * cus, 512)
    if f == 256:
        return (5, 2 * groups // 5 + 7, 256)
    per_clip = 2 * groups // 5 + 2
    return (5, 4 * (per_clip - 1) + 1, 64)


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("f", [256, 64])
def test_the_chunk_walk(gpu_device, f, family):
    cus = _cus(gpu_device)
    shape = _walk_shape(f, cus)
    geom = cc.geometry(shape, cus)
    assert geom["groups"] == min(2 * cus, 512) and 2 * geom["groups"] < geom["chunks"] < 3 * geom["groups"], geom
    assert geom["per_group"] == 3
    if cus == 256:
        assert geom["chunks"] == (1055 if f == 256 else 1030)
    if f == 64:
        assert shape[1] % 4 == 1
    case = cc.make_case(family, shape)
    dw = torch.empty(64, 4, 3, 3, dtype=torch.float32, device=gpu_device) if f == 64 else None      # no store rounding
    _report(f"{family} walk {shape} {geom}", cc.run_checks(case, _run(case, gpu_device, dw=dw), cus))


def test_two_calls_are_bit_identical_on_the_walk(gpu_device):
    case = cc.make_case("dyadic", _walk_shape(64, _cus(gpu_device)), seed=2)
    _all_same(_run(case, gpu_device), _run(case, gpu_device))


# ------------------------------------------------------------------------------------------------- edges

def _zero_input_y(out):
    """What a pooled output over all-zero input is under the call's coefficients: relu(round_bf16(b))."""
    return torch.relu(out["scale_shift"][1].to(BF16))


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("shape", [(2, 5, 16), (2, 3, 64)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("edge", cc.EDGES)
def test_clip_and_frequency_edges(gpu_device, edge, shape, family):
    b, t, f = shape
    case = cc.edge_case(family, shape, edge)
    out = _run(case, gpu_device)
    _report(f"{family} {shape} {edge}", cc.run_checks(case, out, _cus(gpu_device)))
    y = out["y"].view(b, t, f // 2, 64)
    zero = _zero_input_y(out).expand_as(y)
    if edge == "last_row_of_clip_0":                             # nothing of clip 0 reaches clip 1 ...
        assert _same(y[1].contiguous(), zero[1].contiguous())
        assert _same(y[0, :t - 2].contiguous(), zero[0, :t - 2].contiguous())     # ... nor rows beyond the one above
        assert not _same(y[0, t - 1].contiguous(), zero[0, t - 1].contiguous())
    elif edge == "first_column":                                 # bins 0 and 1 see the column: pooled column 0 only
        assert _same(y[:, :, 1:].contiguous(), zero[:, :, 1:].contiguous())
        assert not _same(y[:, :, :1].contiguous(), zero[:, :, :1].contiguous())
    else:
        assert _same(y[:, :, :-1].contiguous(), zero[:, :, :-1].contiguous())
        assert not _same(y[:, :, -1:].contiguous(), zero[:, :, -1:].contiguous())


# ------------------------------------------------------------------------------------------------- weight paths

def _weight_views(w, device):
    """The same bf16 weight values behind every path of cf_load_weights / cf_weight."""
    cl = w.to(device).contiguous(memory_format=CL)
    assert cl.stride() == (36, 1, 12, 4) and cl.data_ptr() % 8 == 0
    buf = torch.zeros(64 * 36 + 4, dtype=BF16, device=device)
    shifted = buf[1:1 + 64 * 36].as_strided((64, 4, 3, 3), (36, 1, 12, 4), 1)   # dense channels-last, 2 bytes off
    shifted.copy_(cl)
    assert shifted.data_ptr() % 8 == 2 and shifted.stride() == cl.stride()
    std = w.to(device).contiguous()
    assert std.stride() == (36, 9, 3, 1)
    return {"bf16 channels-last (packed)": cl, "bf16 channels-last at a 2-byte offset": shifted, "bf16 standard": std,
            "fp32 standard": std.float(), "fp32 channels-last": cl.float()}


@pytest.mark.parametrize("family", FAMILIES)
def test_every_weight_path_gives_the_same_bits(gpu_device, family):
    case = cc.make_case(family, (3, 5, 64), seed=5)
    views = _weight_views(case["w"], gpu_device)
    assert views["fp32 channels-last"].is_contiguous(memory_format=CL)
    outs = {name: _run(case, gpu_device, w=w) for name, w in views.items()}
    first = outs["bf16 channels-last (packed)"]
    _report(f"{family} packed weights", cc.run_checks(case, first, _cus(gpu_device)))
    for name, out in outs.items():
        for k, v in first.items():
            assert _same(v, out[k]), (name, k)


def test_an_inexact_fp32_weight_is_rounded_like_the_cast(gpu_device):
    case = cc.make_case("dyadic", (3, 5, 64), seed=6)
    g = torch.Generator().manual_seed(6)
    w32 = (case["w"].float() * (1 + 2.0 ** -10 * torch.randn(64, 4, 3, 3, generator=g))).to(gpu_device)
    assert not torch.equal(w32.bfloat16().float(), w32)
    _all_same(_run(case, gpu_device, w=w32), _run(case, gpu_device, w=w32.bfloat16()))
    _all_same(_run(case, gpu_device, w=w32.contiguous(memory_format=CL)), _run(case, gpu_device, w=w32.bfloat16()))


# ------------------------------------------------------------------------------------------------- C ABI

def _ptr(t):
    return None if t is None else t.data_ptr()


def _forward_args(x, w, gamma, beta, rm, rv, momentum, eps, y, mi, ss, ws, phases=3):
    b, _, t, f = x.shape
    return [_ptr(x), _ptr(w), int(w.dtype == BF16), *w.stride(), b, t, f, _ptr(gamma), _ptr(beta), _ptr(rm), _ptr(rv),
            momentum, eps, _ptr(y), _ptr(mi), _ptr(ss), _ptr(ws), phases, None]


def _backward_args(x, w, dy, mi, ss, dw, dgamma, dbeta, ws, phases=3):
    b, _, t, f = x.shape
    return [_ptr(x), _ptr(w), int(w.dtype == BF16), *w.stride(), _ptr(dy), b, t, f, _ptr(mi), _ptr(ss), _ptr(dw),
            int(dw.dtype == BF16), *dw.stride(), _ptr(dgamma), _ptr(dbeta), _ptr(ws), phases, None]


class _Call:
    """Device tensors of one case for calls through the C ABI by address; outputs filled with sentinels."""

    def __init__(self, case, device, guard=4096):
        import seld_native
        seld_native.ensure_init(device)
        self.lib = seld_native.load_library()
        b, t, f = case["shape"]
        self.case, self.device, self.guard, self.n_y = case, device, guard, b * t * (f // 2) * 64
        self.x = case["x"].to(device).contiguous(memory_format=CL)
        self.dy = case["dy"].to(device).contiguous(memory_format=CL)
        self.w = case["w"].to(device).contiguous(memory_format=CL)
        self.gamma, self.beta = case["weight"].to(device), case["bias"].to(device)
        self.ws = torch.zeros(int(self.lib.seld_convfirst_workspace_floats(1)), dtype=torch.float32, device=device)
        self.reset()

    def reset(self):
        d = self.device
        self.rm, self.rv = self.case["rm0"].to(d), self.case["rv0"].to(d)
        self.ypat = (torch.arange(self.n_y + 2 * self.guard, dtype=torch.int32) % 251 + 0x3F00).to(torch.int16).to(d)
        self.ybuf = self.ypat.clone()
        self.y = self.ybuf[self.guard:self.guard + self.n_y].view(BF16)
        self.stats = torch.full((2, 2, 64), -7.0, device=d)
        self.dgb = torch.full((2, 64), -7.0, device=d)
        self.dw = torch.full((64, 4, 3, 3), -7.0, dtype=BF16, device=d).contiguous(memory_format=CL)

    def forward(self, phases=3, **override):
        a = dict(x=self.x, w=self.w, gamma=self.gamma, beta=self.beta, rm=self.rm, rv=self.rv,
                 momentum=self.case["momentum"], eps=self.case["eps"], y=self.y, mi=self.stats[0], ss=self.stats[1],
                 ws=self.ws, phases=phases)
        a.update(override)
        return self.lib.seld_convfirst_forward(*_forward_args(**a))

    def backward(self, phases=3, **override):
        a = dict(x=self.x, w=self.w, dy=self.dy, mi=self.stats[0], ss=self.stats[1], dw=self.dw, dgamma=self.dgb[0],
                 dbeta=self.dgb[1], ws=self.ws, phases=phases)
        a.update(override)
        return self.lib.seld_convfirst_backward(*_backward_args(**a))

    def outputs(self):
        torch.cuda.synchronize()
        b, t, f = self.case["shape"]
        return dict(y=self.y.view(b * t * (f // 2), 64).cpu(), mean_invstd=self.stats[0].cpu(),
                    scale_shift=self.stats[1].cpu(), running_mean=self.rm.cpu(), running_var=self.rv.cpu(),
                    dw=self.dw.cpu().contiguous(), dgamma=self.dgb[0].cpu(), dbeta=self.dgb[1].cpu())

    def untouched(self):
        """True when no output holds anything but its sentinel and the running statistics are the case's."""
        torch.cuda.synchronize()
        return (torch.equal(self.ybuf, self.ypat) and bool((self.stats == -7.0).all()) and bool((self.dgb == -7.0).all())
                and bool((self.dw.float() == -7.0).all()) and torch.equal(self.rm.cpu(), self.case["rm0"])
                and torch.equal(self.rv.cpu(), self.case["rv0"]))


DW_LAYOUTS = ["channels_last", "standard", "slice"]


def _dw_target(layout, dtype, device, guard=512):
    """A [64, 4, 3, 3] gradient tensor of ``dtype`` inside a sentinel-filled buffer: ``guard`` elements on either side
    and, for "slice", columns 1 .. 3 of a [64, 4, 3, 5] buffer (two sentinel columns in every row of taps).
    -> (tensor, buffer, pattern copy, mask of the buffer elements that belong to the tensor)."""
    span = 64 * 4 * 3 * 5 if layout == "slice" else 64 * 36
    ints = torch.int16 if dtype == BF16 else torch.int32
    pattern = (torch.arange(span + 2 * guard, dtype=torch.int32) % 251 + 0x3F00).to(ints).to(device)
    buf = pattern.clone()
    strides, offset = {"channels_last": ((36, 1, 12, 4), guard), "standard": ((36, 9, 3, 1), guard),
                       "slice": ((60, 15, 5, 1), guard + 1)}[layout]
    dw = buf.view(dtype).as_strided((64, 4, 3, 3), strides, offset)
    mask = torch.zeros(span + 2 * guard, dtype=torch.bool, device=device)
    mask.as_strided((64, 4, 3, 3), strides, offset).fill_(True)
    assert int(mask.sum()) == 64 * 36
    return dw, buf, pattern, mask


@pytest.mark.parametrize("dtype", [BF16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("layout", DW_LAYOUTS)
def test_writes_nothing_outside_y_and_dw(gpu_device, layout, dtype):
    """Ragged T (11 rows, 8 per chunk).  y is a slice of a sentinel buffer with guards, dw a strided view of one, both
    passed by address: guards and gaps come back bit-identical, and the slices hold what the wrappers return and what
    the replay demands."""
    case = cc.make_case("dyadic", (2, 11, 32), seed=7)
    call = _Call(case, gpu_device)
    dw, buf, pattern, mask = _dw_target(layout, dtype, gpu_device)
    dense = torch.empty(64, 4, 3, 3, dtype=dtype, device=gpu_device)
    want = _run(case, gpu_device, dw=dense.contiguous(memory_format=CL) if layout == "channels_last" else dense)
    assert call.forward() == 0
    assert call.backward(dw=dw) == 0
    out = call.outputs()
    out["dw"] = dw.cpu().contiguous()
    g, n = call.guard, call.n_y
    assert torch.equal(call.ybuf[:g], call.ypat[:g]) and torch.equal(call.ybuf[g + n:], call.ypat[g + n:])
    assert torch.equal(buf[~mask], pattern[~mask])
    assert bool((call.dw.float() == -7.0).all())                 # the call's own dw was not the target
    _all_same(want, out)
    _report(f"dw {layout} {dtype}", cc.run_checks(case, out, _cus(gpu_device)))


@pytest.mark.parametrize("family", FAMILIES)
def test_phases_one_then_two_equal_three(gpu_device, family):
    """On one caller-held workspace: statistics pass, then finalise + apply; reduce pass, then finalise + wgrad + sum."""
    case = cc.make_case(family, (3, 5, 64), seed=8)
    whole = _Call(case, gpu_device)
    assert whole.forward(3) == 0 and whole.backward(3) == 0
    want = whole.outputs()
    split = _Call(case, gpu_device)
    assert split.forward(1) == 0
    torch.cuda.synchronize()
    assert torch.equal(split.ybuf, split.ypat) and bool((split.stats == -7.0).all())      # phase 1 writes partials only
    assert torch.equal(split.rm.cpu(), case["rm0"]) and torch.equal(split.rv.cpu(), case["rv0"])
    assert split.forward(2) == 0
    assert split.backward(1) == 0
    torch.cuda.synchronize()
    assert bool((split.dgb == -7.0).all()) and bool((split.dw.float() == -7.0).all())
    assert split.backward(2) == 0
    _all_same(want, split.outputs())
    _report(f"{family} phases", cc.run_checks(case, want, _cus(gpu_device)))


def test_refusals_write_nothing(gpu_device):
    case = cc.make_case("integer", (2, 3, 16), seed=9)
    call = _Call(case, gpu_device)
    off = lambda t, n: _Shaped(t, t.shape, 2 * n)                # the same storage n bf16 elements further on
    assert off(call.x, 1).data_ptr() % 8 == 2 and off(call.x, 2).data_ptr() % 8 == 4
    for n in (1, 2):
        assert call.forward(x=off(call.x, n)) == INVALID
        assert call.forward(y=off(call.y, n)) == INVALID
        assert call.backward(x=off(call.x, n)) == INVALID
        assert call.backward(dy=off(call.dy, n)) == INVALID
    for name in ("x", "gamma", "beta", "rm", "rv", "y", "mi", "ss", "ws"):
        assert call.forward(**{name: _Null(call.x.shape) if name == "x" else None}) == INVALID, name
    for name in ("x", "dy", "mi", "ss", "dgamma", "dbeta", "ws"):
        assert call.backward(**{name: _Null(call.x.shape) if name == "x" else None}) == INVALID, name
    assert call.backward(dw=_NullLike(call.dw)) == INVALID and call.backward(w=_NullLike(call.w)) == INVALID
    assert call.forward(w=_NullLike(call.w)) == INVALID
    for b, t in ((0, 3), (-1, 3), (2, 0), (2, -5)):
        shaped = _Shaped(call.x, (b, 4, t, 16))
        assert call.forward(x=shaped) == INVALID and call.backward(x=shaped) == INVALID, (b, t)
    for f in (8, 48, 512):
        shaped = _Shaped(call.x, (2, 4, 3, f))
        assert call.forward(x=shaped) == UNSUPPORTED and call.backward(x=shaped) == UNSUPPORTED, f
    assert call.untouched()
    assert call.forward() == 0 and call.backward() == 0          # and the same call object does run
    _report("after the refusals", cc.run_checks(case, call.outputs(), _cus(gpu_device)))


class _Shaped:
    """A tensor's address, plus ``offset`` bytes, under another shape (the C ABI takes B, T, F as numbers)."""

    def __init__(self, t, shape, offset=0):
        self.t, self.shape, self.offset = t, tuple(shape), offset

    def data_ptr(self):
        return self.t.data_ptr() + self.offset


class _Null:
    def __init__(self, shape):
        self.shape = tuple(shape)

    def data_ptr(self):
        return None


class _NullLike:
    """A null pointer with a tensor's dtype and strides."""

    def __init__(self, t):
        self.dtype, self._stride = t.dtype, t.stride()

    def stride(self):
        return self._stride

    def data_ptr(self):
        return None
