"""The BiGRU recurrence kernels (csrc/gru.hip) on 2-sequence tiles against the 4-sequence build they replace.

The arithmetic of one sequence does not depend on its MFMA column neighbours, so y, dgi and dghn of any tile geometry
must be, bit for bit, what the build before 2-sequence tiles were admitted wrote for the same seeded operands:
tests/golden/gru_tile4_parent.npz, recorded on that build by tools/record_gru_parent_golden.py (bf16 bit patterns).
Only the bias gradients may differ: fp32 sums of the same B*T terms per (direction, slot, unit), grouped by tile.

Shapes (B, T), tests/gru_tile2_cases.py: (1, 1), (2, 2), (3, 5), (5, 4), (9, 7) -- a batch smaller than a tile, odd
batches whose last tile has a padding sequence, T = 1 (the peeled step only), T = 2 (no loop trip), odd and even
numbers of loop trips.  H = 256.  Every test runs the library as built by default."""
import functools
from pathlib import Path

import numpy as np
import pytest
import torch

import gru_tile2_cases as cases

pytestmark = pytest.mark.gpu
H = cases.H
FIXTURE = Path(__file__).resolve().parent / "golden" / "gru_tile4_parent.npz"


@functools.lru_cache(maxsize=None)
def golden():
    with np.load(FIXTURE) as z:
        return {k: z[k] for k in z.files}


def from_bits(a, device):
    return torch.from_numpy(a.view(np.int16)).to(device).view(torch.bfloat16)


_results = {}


def result(device, batch, steps):
    """One forward / direct backward / bias reduction per shape, shared by the tests below and left unchanged."""
    import seld_native as nat
    if (batch, steps) not in _results:
        _results[(batch, steps)] = cases.run(nat, device, batch, steps)
    return _results[(batch, steps)]


@pytest.mark.parametrize("batch,steps", cases.SHAPES)
def test_outputs_are_bit_identical_to_the_4_sequence_build(gpu_device, batch, steps):
    y, dgi, dghn, _, _ = result(gpu_device, batch, steps)
    ref = golden()
    for name, got in (("y", y), ("dgi", dgi), ("dghn", dghn)):
        want = from_bits(ref[cases.key(batch, steps, name)], gpu_device)
        assert tuple(got.shape) == tuple(want.shape), name
        assert torch.equal(got.contiguous(), want), name
    assert dgi.float().abs().max().item() > 0


@pytest.mark.parametrize("batch,steps", cases.SHAPES)
def test_bias_gradients_within_the_reordering_bound(gpu_device, batch, steps):
    """|db_new - db_golden| <= 2 N 2^-24 1.01 sum_{b,t} |dg| per element, N = B T: both are fp32 sums of the same N
    terms in different groupings (each within N 2^-24 sum|dg| of the exact sum, to first order); sum|dg| is taken from
    the stored bf16 dgi / dghn (identical to the golden ones, see above) and 1.01 covers their rounding (2^-8 relative)."""
    _, dgi, dghn, db_ih, db_hh = result(gpu_device, batch, steps)
    ref = golden()
    n = batch * steps
    mag_gi = dgi.float().abs().sum(dim=(0, 1))                                  # [2, 3, H]
    mag_n = dghn.float().abs().sum(dim=(0, 1))                                  # [2, H]
    mag_ih = mag_gi.reshape(-1)
    mag_hh = torch.cat((mag_gi[:, :2], mag_n[:, None]), dim=1).reshape(-1)      # db_hh = (r, z, n r)
    for name, got, mag in (("db_ih", db_ih, mag_ih), ("db_hh", db_hh, mag_hh)):
        want = torch.from_numpy(ref[cases.key(batch, steps, name)]).to(gpu_device)
        bound = 2.0 * n * 2.0 ** -24 * 1.01 * mag
        err = (got.double() - want.double()).abs()
        print(f"{name} B={batch} T={steps}: max err {err.max().item():.3e}, max err/bound "
              f"{(err / bound.clamp_min(1e-30)).max().item():.3f}")
        assert torch.isfinite(got).all() and (err <= bound.double()).all(), name


GUARD = 3                                                                       # rows in front of and behind the result


def _guarded(rows, tail, dtype, device):
    """A NaN-filled buffer of GUARD + rows + GUARD rows and the view of its middle rows."""
    big = torch.full((rows + 2 * GUARD,) + tail, float("nan"), dtype=dtype, device=device)
    return big, big[GUARD:GUARD + rows]


def _guards_untouched(big, rows):
    return bool(torch.isnan(big[:GUARD]).all() and torch.isnan(big[GUARD + rows:]).all())


@pytest.mark.parametrize("batch,steps", [(3, 5), (5, 4)])
def test_nothing_outside_the_batch_is_read_into_a_result_or_written(gpu_device, batch, steps):
    """Through the C ABI on the caller's buffers.  Forward: gi is exactly B rows in a NaN-filled buffer (a padding
    sequence that read past it would save NaN gates), y is the tile-padded row count in one (the 4-byte-per-lane copy
    of the h tile by half of the wavefronts must write those rows and nothing else).  Backward: dy / y are exactly B
    rows between NaN rows, dgi / dghn exactly B rows between NaN guards (the copy-out predicate)."""
    import seld_native as nat
    lib, P, st = nat.load_library(), nat._p, nat._stream_ptr(gpu_device)
    seqs = nat.GRU_TILE
    tiles = (batch + seqs - 1) // seqs
    gi, w_hh, b_hn, dy = cases.recurrence_case(batch, steps)
    ref = golden()
    w = w_hh.to(gpu_device).to(torch.bfloat16).contiguous()
    w_t = w.transpose(1, 2).contiguous()
    bias = b_hn.to(gpu_device)

    big_gi, gi_d = _guarded(batch, (steps, 2, 3 * H), torch.bfloat16, gpu_device)
    gi_d.copy_(gi)
    big_y, y = _guarded(tiles * seqs, (steps, 2 * H), torch.bfloat16, gpu_device)
    saved = torch.full((tiles, steps, 2, 8, 2, 64, 2, 8 * seqs // 16), float("nan"), dtype=torch.float16,
                       device=gpu_device)
    nat.check(lib.seld_gru_forward(P(gi_d), 1, P(w), P(bias), batch, steps, H, P(y), P(saved), st), "seld_gru_forward")
    torch.cuda.synchronize(gpu_device)
    assert _guards_untouched(big_y, tiles * seqs)
    assert torch.isfinite(y.float()).all() and torch.isfinite(saved.float()).all()
    want_y = from_bits(ref[cases.key(batch, steps, "y")], gpu_device)
    assert torch.equal(y[:batch], want_y)

    big_dy, dy_d = _guarded(batch, (steps, 2 * H), torch.bfloat16, gpu_device)
    dy_d.copy_(dy)
    big_yin, y_in = _guarded(batch, (steps, 2 * H), torch.bfloat16, gpu_device)
    y_in.copy_(want_y)
    big_dgi, dgi = _guarded(batch, (steps, 2, 3, H), torch.bfloat16, gpu_device)
    big_dghn, dghn = _guarded(batch, (steps, 2, H), torch.bfloat16, gpu_device)
    dbias = torch.full((tiles, 2, 4, H), float("nan"), dtype=torch.float32, device=gpu_device)
    nat.check(lib.seld_gru_backward_direct(P(dy_d), P(saved), P(y_in), 1, P(w_t), batch, steps, H, P(dgi), P(dghn),
                                           P(dbias), st), "seld_gru_backward_direct")
    torch.cuda.synchronize(gpu_device)
    assert _guards_untouched(big_dgi, batch) and _guards_untouched(big_dghn, batch)
    assert torch.isfinite(dgi.float()).all() and torch.isfinite(dghn.float()).all() and torch.isfinite(dbias).all()
    assert torch.equal(dgi, from_bits(ref[cases.key(batch, steps, "dgi")], gpu_device))
    assert torch.equal(dghn, from_bits(ref[cases.key(batch, steps, "dghn")], gpu_device))


def test_captured_replay_equals_eager(gpu_device):
    """One SeldGRU layer at (5, 4) under bf16 autocast, forward and backward, eager and as a replayed capture.  The pass
    is run the way the captured training step runs it (tests/test_gru_direct_gpu.py::_module_grads): the layer's
    parameter gradients on a side stream, joined after the pass, so the capture has the fork and join every capture of
    this project has; y leaves through a buffer allocated outside the capture."""
    import seld_gru
    import seld_overlap
    from seld_rnn import SeldGRU
    assert seld_overlap.enabled
    batch, steps = 5, 4
    torch.manual_seed(31)
    m = SeldGRU(input_size=96, hidden_size=H, num_layers=1, batch_first=True, bidirectional=True).to(gpu_device).train()
    x = torch.randn(batch, steps, 96, device=gpu_device)
    go = torch.randn(batch, steps, 2 * H, device=gpu_device)
    xin = x.clone().requires_grad_(True)
    y_out = torch.zeros(batch, steps, 2 * H, dtype=torch.bfloat16, device=gpu_device)

    def run():
        for p in m.parameters():
            p.grad = None
        xin.grad = None
        seld_overlap.conv_wgrad_side = True
        try:
            with torch.autocast("cuda", dtype=torch.bfloat16):
                y, _ = seld_gru.bigru_forward(m, xin, overlap=True, need_hn=False)
            torch.autograd.backward(y, go.to(y.dtype))
            with torch.no_grad():
                y_out.copy_(y)
        finally:
            seld_overlap.conv_wgrad_side = False
            seld_overlap.join(gpu_device)

    def collect():
        torch.cuda.synchronize(gpu_device)
        grads = {"y": y_out.clone(), "dx": xin.grad.clone()}
        grads.update({name: p.grad.clone() for name, p in m.named_parameters()})
        return grads

    run()
    eager = collect()

    side = torch.cuda.Stream(device=gpu_device)
    side.wait_stream(torch.cuda.current_stream(gpu_device))
    with torch.cuda.stream(side):
        for _ in range(3):                                        # warm-up: library workspaces, kernel selections
            run()
    torch.cuda.current_stream(gpu_device).wait_stream(side)
    torch.cuda.synchronize(gpu_device)
    captured = torch.cuda.CUDAGraph()
    with torch.no_grad():
        xin.copy_(torch.zeros_like(x))                            # the capture executes nothing: the replay must see x
    with torch.cuda.graph(captured):
        run()
    with torch.no_grad():
        xin.copy_(x)
        y_out.fill_(float("nan"))
        for p in m.parameters():                                  # a gradient the replay does not rewrite shows as NaN
            p.grad.fill_(float("nan"))
    captured.replay()
    replay = collect()
    assert len(eager) == 2 + 8
    for name, want in eager.items():
        assert torch.isfinite(want.float()).all() and want.float().abs().max().item() > 0, name
        assert torch.equal(replay[name], want), name
