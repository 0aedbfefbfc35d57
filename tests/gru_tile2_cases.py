"""Seeded operands and the recorded-result keys shared by tools/record_gru_parent_golden.py and
tests/test_gru_tile2_gpu.py (no test in here)."""
import torch

H = 256
SEED = 12
# (B, T): a batch smaller than a tile; T = 1 (the peeled step only); T = 2 (no loop trip); odd batches whose last tile
# has a padding sequence; an even (T = 5: two) and an odd (T = 4: one, T = 7: three) number of loop trips
SHAPES = [(1, 1), (2, 2), (3, 5), (5, 4), (9, 7)]


def recurrence_case(batch, steps, seed=SEED):
    """The seeded operands of tests/test_gru_direct_gpu.py::_recurrence_case."""
    g = torch.Generator().manual_seed(seed)
    k = 1.0 / H ** 0.5
    gi = (torch.randn(batch, steps, 2, 3 * H, generator=g) * 1.2).to(torch.bfloat16)
    w_hh = (torch.rand(2, 3 * H, H, generator=g) * 2 - 1) * 2 * k
    b_hn = (torch.rand(2, H, generator=g) * 2 - 1) * k
    dy = (torch.randn(batch, steps, 2 * H, generator=g) * 0.5).to(torch.bfloat16)
    return gi, w_hh, b_hn, dy


def key(batch, steps, what):
    return f"b{batch}_t{steps}_{what}"


def run(nat, device, batch, steps):
    """gru_forward -> gru_backward(direct=True) -> gru_bias_grads on the seeded case: device tensors
    (y, dgi, dghn, db_ih, db_hh)."""
    gi, w_hh, b_hn, dy = recurrence_case(batch, steps)
    w = w_hh.to(device)
    y, saved = nat.gru_forward(gi.to(device), w, b_hn.to(device), True)
    dgi, dghn, partial = nat.gru_backward(dy.to(device), saved, y.contiguous(), w, raw_bias=True, direct=True)
    db_ih, db_hh = nat.gru_bias_grads(partial.contiguous())
    torch.cuda.synchronize(device)
    return y, dgi, dghn, db_ih, db_hh
