"""The direct-layout backward recurrence (csrc/gru.hip, ``gru_backward_kernel<bf16, true>``; ``seld_gru_backward_direct``)
and the parameter-only prepare launch (``seld_gru_prepare``) against what they replace.

The direct kernel runs the tile kernel's arithmetic unchanged -- same MFMA chains, same order of every sum, same bf16
roundings of what is stored -- and differs only in where dy is read from and where the gate gradients are written, so
every comparison here is ``torch.equal``: no tolerance to derive.  Shapes: a single step, partly filled tiles with even
and odd T, the two-step loop's odd tail, ten ragged tiles.  The workload size (32, 250) runs through the same kernel in
tests/test_gru_gpu.py.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu
H = 256
SHAPES = [(1, 1), (3, 2), (5, 7), (6, 41), (9, 5), (37, 20)]


def _recurrence_case(batch, steps, seed):
    """The seeded operands of tests/test_gru_gpu.py::_recurrence_case."""
    g = torch.Generator().manual_seed(seed)
    k = 1.0 / H ** 0.5
    gi = (torch.randn(batch, steps, 2, 3 * H, generator=g) * 1.2).to(torch.bfloat16)
    w_hh = (torch.rand(2, 3 * H, H, generator=g) * 2 - 1) * 2 * k
    b_hn = (torch.rand(2, H, generator=g) * 2 - 1) * k
    dy = (torch.randn(batch, steps, 2 * H, generator=g) * 0.5).to(torch.bfloat16)
    return gi, w_hh, b_hn, dy


def _tile_path(nat, dy, saved, y, w_t):
    """to_tile_device -> seld_gru_backward -> from_pair_tile_device through the bindings: (dgi, dghn, raw dbias)."""
    b, t, _ = dy.shape
    seqs = nat.GRU_TILE
    dy_tile = nat.to_tile_device(dy.reshape(b, t, 2, 1, H), 1)
    tiles = dy_tile.shape[0]
    if tiles * seqs != b:
        y = torch.cat((y, y.new_zeros((tiles * seqs - b, t, 2 * H))), dim=0)
    y = y.contiguous()
    dg_tile = torch.empty((tiles, t, 2, 8, 2, 4, 16 // seqs, seqs, 2, seqs // 2), dtype=dy.dtype, device=dy.device)
    dbias = torch.full((tiles, 2, 4, H), float("nan"), dtype=torch.float32, device=dy.device)
    P = nat._p
    nat.check(nat.load_library().seld_gru_backward(P(dy_tile), P(saved), P(y), 1, P(w_t), tiles, t, H, P(dg_tile),
                                                   P(dbias), nat._stream_ptr(dy.device)), "seld_gru_backward")
    dgi, dghn = nat.from_pair_tile_device(dg_tile, b)
    return dgi, dghn, dbias


def _direct(nat, dy, saved, y, w_t, dgi, dghn):
    """seld_gru_backward_direct on the caller's tensors (views of exactly B rows): raw dbias."""
    b, t, _ = dy.shape
    tiles = (b + nat.GRU_TILE - 1) // nat.GRU_TILE
    dbias = torch.full((tiles, 2, 4, H), float("nan"), dtype=torch.float32, device=dy.device)
    P = nat._p
    nat.check(nat.load_library().seld_gru_backward_direct(P(dy), P(saved), P(y), 1, P(w_t), b, t, H, P(dgi), P(dghn),
                                                          P(dbias), nat._stream_ptr(dy.device)),
              "seld_gru_backward_direct")
    return dbias


_cases = {}


def _case(device, batch, steps):
    """Forward once and the tile path's backward once per shape; shared by the tests below and left unchanged."""
    import seld_native as nat
    key = (batch, steps)
    if key not in _cases:
        gi, w_hh, b_hn, dy = _recurrence_case(batch, steps, 12)
        w = w_hh.to(device)
        y, saved = nat.gru_forward(gi.to(device), w, b_hn.to(device), True)
        w_t = w.to(torch.bfloat16).transpose(1, 2).contiguous()
        dy = dy.to(device)
        _cases[key] = (dy, saved, y.contiguous(), w_t, _tile_path(nat, dy, saved, y, w_t))
    return _cases[key]


@pytest.mark.parametrize("batch,steps", SHAPES)
def test_direct_backward_is_bit_identical_to_the_tile_path(gpu_device, batch, steps):
    import seld_native as nat
    dy, saved, y, w_t, (ref_gi, ref_n, ref_b) = _case(gpu_device, batch, steps)
    assert torch.isfinite(ref_b).all() and ref_gi.float().abs().max().item() > 0
    outs = []
    for _ in range(2):
        dgi = torch.empty((batch, steps, 2, 3, H), dtype=torch.bfloat16, device=gpu_device)
        dghn = torch.empty((batch, steps, 2, H), dtype=torch.bfloat16, device=gpu_device)
        outs.append((dgi, dghn, _direct(nat, dy, saved, y, w_t, dgi, dghn)))
    for dgi, dghn, dbias in outs:
        assert torch.equal(dgi, ref_gi) and torch.equal(dghn, ref_n) and torch.equal(dbias, ref_b)
    # the Python entry takes the same route for bf16 and keeps the converters for ``direct=False``
    a = nat.gru_backward(dy, saved, y, None, raw_bias=True, w_hh_t=w_t)
    b = nat.gru_backward(dy, saved, y, None, raw_bias=True, w_hh_t=w_t, direct=False)
    for got_a, got_b, want in zip(a, b, (ref_gi, ref_n, ref_b)):
        assert torch.equal(got_a, want) and torch.equal(got_b, want)


def test_direct_export_is_bf16_only(gpu_device):
    import seld_native as nat
    dy, saved, y, w_t, _ = _case(gpu_device, 3, 2)
    dgi = torch.empty((3, 2, 2, 3, H), dtype=torch.bfloat16, device=gpu_device)
    dghn = torch.empty((3, 2, 2, H), dtype=torch.bfloat16, device=gpu_device)
    dbias = torch.empty((1, 2, 4, H), dtype=torch.float32, device=gpu_device)
    P = nat._p
    rc = nat.load_library().seld_gru_backward_direct(P(dy), P(saved), P(y), 0, P(w_t), 3, 2, H, P(dgi), P(dghn), P(dbias),
                                                     nat._stream_ptr(gpu_device))
    assert rc == -4                                               # SELD_ERR_UNSUPPORTED (include/seld_hip.h)


SENTINEL = 0x5A5A


@pytest.mark.parametrize("batch,steps", SHAPES)
def test_direct_backward_stays_inside_the_batch(gpu_device, batch, steps):
    """dgi / dghn are the leading B rows of larger buffers filled with a sentinel bit pattern: the rows behind them stay
    untouched.  dy / y are the leading B rows of buffers whose further rows are NaN: a padding sequence of the last tile
    that read them would carry NaN into dbias (and a NaN times its zero dy would still be NaN)."""
    import seld_native as nat
    dy, saved, y, w_t, (ref_gi, ref_n, ref_b) = _case(gpu_device, batch, steps)
    extra = 5                                                     # more than a tile's padding rows
    big_gi = torch.full((batch + extra, steps, 2, 3, H), SENTINEL, dtype=torch.int16, device=gpu_device)
    big_n = torch.full((batch + extra, steps, 2, H), SENTINEL, dtype=torch.int16, device=gpu_device)
    big_dy = torch.full((batch + extra, steps, 2 * H), float("nan"), dtype=torch.bfloat16, device=gpu_device)
    big_y = torch.full((batch + extra, steps, 2 * H), float("nan"), dtype=torch.bfloat16, device=gpu_device)
    big_dy[:batch] = dy
    big_y[:batch] = y
    dgi, dghn = big_gi.view(torch.bfloat16)[:batch], big_n.view(torch.bfloat16)[:batch]
    dbias = _direct(nat, big_dy[:batch], saved, big_y[:batch], w_t, dgi, dghn)
    assert (big_gi[batch:] == SENTINEL).all() and (big_n[batch:] == SENTINEL).all()
    assert torch.isfinite(dbias).all() and torch.isfinite(dgi.float()).all() and torch.isfinite(dghn.float()).all()
    assert torch.equal(dgi, ref_gi) and torch.equal(dghn, ref_n) and torch.equal(dbias, ref_b)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("w_dtype", [torch.float32, torch.bfloat16])
def test_prepare_matches_fold_bias_and_the_torch_transpose(gpu_device, dtype, w_dtype):
    import seld_native as nat
    g = torch.Generator().manual_seed(21)
    b_ih = (torch.rand(6 * H, generator=g) - 0.5).to(gpu_device)
    b_hh = (torch.rand(6 * H, generator=g) - 0.5).to(gpu_device)
    w_hh = ((torch.rand(2, 3 * H, H, generator=g) * 2 - 1) / 8).to(w_dtype).to(gpu_device)
    gi_bias, b_hn, w_t = nat.gru_prepare(b_ih, b_hh, w_hh, dtype)
    ref_bias, ref_hn = nat.gru_fold_bias(b_ih, b_hh, dtype)
    assert gi_bias.dtype == dtype and torch.equal(gi_bias, ref_bias) and torch.equal(b_hn, ref_hn)
    assert w_t.dtype == torch.bfloat16 and torch.equal(w_t, w_hh.to(torch.bfloat16).transpose(1, 2).contiguous())


def _module_grads(m, x, go, device, graph):
    """One forward / backward of the 2-layer module as the captured step runs it: layer 1's parameter gradients
    submitted to side stream 0, layer 0's launched on side stream 1, joined after the pass."""
    import seld_gru
    import seld_overlap
    xin = x.clone().requires_grad_(True)
    go = go.clone()

    def run():
        for p in m.parameters():
            p.grad = None
        xin.grad = None
        seld_overlap.conv_wgrad_side = True
        try:
            with torch.autocast("cuda", dtype=torch.bfloat16):
                y, _ = seld_gru.bigru_forward(m, xin, overlap=True, need_hn=False)
            torch.autograd.backward(y, go.to(y.dtype))
        finally:
            seld_overlap.conv_wgrad_side = False
            seld_overlap.join(device)

    if not graph:
        run()
    else:
        side = torch.cuda.Stream(device=device)
        side.wait_stream(torch.cuda.current_stream(device))
        with torch.cuda.stream(side):
            for _ in range(3):                                    # warm-up: library workspaces, kernel selections
                run()
        torch.cuda.current_stream(device).wait_stream(side)
        torch.cuda.synchronize(device)
        captured = torch.cuda.CUDAGraph()
        with torch.no_grad():
            xin.copy_(torch.zeros_like(x))                        # the capture executes nothing: the replay must see x
        with torch.cuda.graph(captured):
            run()
        with torch.no_grad():
            xin.copy_(x)
            for p in m.parameters():                              # a gradient the replay does not rewrite shows as NaN
                p.grad.fill_(float("nan"))
        captured.replay()
    torch.cuda.synchronize(device)
    grads = {"dx": xin.grad.clone()}
    grads.update({name: p.grad.clone() for name, p in m.named_parameters()})
    return grads


def test_module_gradients_eager_captured_and_without_the_direct_path(gpu_device):
    """SeldGRU (2 layers) under bf16 autocast: dx and all parameter gradients of both layers are equal between the eager
    pass, the replayed capture (bias gradients produced by the side-stream jobs) and the pass with the direct path off."""
    import seld_gru
    import seld_overlap
    from seld_rnn import SeldGRU
    assert seld_overlap.enabled
    torch.manual_seed(8)
    m = SeldGRU(input_size=96, hidden_size=H, num_layers=2, batch_first=True, bidirectional=True).to(gpu_device).train()
    x = torch.randn(6, 41, 96, device=gpu_device)
    go = torch.randn(6, 41, 2 * H, device=gpu_device)
    assert seld_gru.direct_backward
    eager = _module_grads(m, x, go, gpu_device, graph=False)
    replay = _module_grads(m, x, go, gpu_device, graph=True)
    seld_gru.direct_backward = False
    try:
        tile = _module_grads(m, x, go, gpu_device, graph=False)
    finally:
        seld_gru.direct_backward = True
    assert len(eager) == 1 + 16
    for name, want in eager.items():
        assert torch.isfinite(want).all() and want.abs().max().item() > 0, name
        assert torch.equal(replay[name], want), name
        assert torch.equal(tile[name], want), name
