"""The cases shared by tools/record_bf16_sites_golden.py, tests/test_bf16_sites_gpu.py and tests/test_bf16_sites_cpu.py
(no test in here): every bf16 store of csrc/ that no other test compares bit for bit, run once on seeded inputs.

Pass-through sites get the rounding family; computed sites get seeded normal inputs at the smallest shape their entry
point takes (the losses: one full 256-cell tile plus a ragged one, so that the 16-byte and the pair store both run).
Not in here, because an existing test already requires equal bits: the conv tails, the first block, the depthwise conv
and LayerNorm (float64 replay tests), the conv loop (test_conv_loop_parent_bits_gpu.py), the GRU recurrences
(test_gru_tile2_gpu.py), and conv_weight_flip_transpose, which moves bits without converting
(test_glue_gpu.py compares it with torch.equal)."""
import numpy as np
import torch

SEED = 41
_H = (0x0000, 0x0001, 0x007F, 0x0080, 0x3F80, 0x3F81, 0x7F7F, 0x7F80)
HIGH = _H + tuple(h | 0x8000 for h in _H)                  # the kept half, both signs
LOW = (0x0000, 0x0001, 0x7FFF, 0x8000, 0x8001, 0xFFFF)     # the discarded half
ADAM = dict(beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0)


def family_bits() -> np.ndarray:
    """uint32 [96]: h << 16 | l, h-major."""
    return np.array([(h << 16) | l for h in HIGH for l in LOW], dtype=np.uint32)


def family(length: int) -> torch.Tensor:
    """fp32 [length]: the family repeated."""
    bits = np.resize(family_bits(), length)
    return torch.from_numpy(bits.view(np.int32).copy()).view(torch.float32)


# the 8-wide body alone (one whole chunk of the cast kernel), and the body plus a scalar tail of 3 in a second block
LENGTHS = (8192, 8195)


def bits(x: torch.Tensor) -> np.ndarray:
    return x.contiguous().view(torch.int16).cpu().numpy().view(np.uint16).reshape(-1)


def _normal(g, *shape, scale=1.0):
    return torch.randn(*shape, generator=g) * scale


def _adam(nat, dev, guarded):
    out = {}
    for n in LENGTHS:
        p = family(n).to(dev)
        low = torch.zeros(n, dtype=torch.bfloat16, device=dev)
        zeros = [torch.zeros(n, device=dev) for _ in range(3)]
        lr, step = torch.full((1,), 1e-3, device=dev), torch.ones(1, device=dev)
        fn = nat.multi_adam_guarded if guarded else nat.multi_adam
        assert fn([zeros[0]], [p], [zeros[1]], [zeros[2]], [low], lr, step, **ADAM)
        out[f"{'adam_guarded' if guarded else 'adam'}_{n}"] = low
    return out


def run(nat, dev) -> dict:
    """{name: bf16 device tensor} of every case, on the library ``nat`` has loaded."""
    out = {}
    g = torch.Generator().manual_seed(SEED)

    # ---- pass-through sites
    for n in LENGTHS:
        dst = torch.zeros(n, dtype=torch.bfloat16, device=dev)
        assert nat.multi_cast([family(n).to(dev)], [dst])
        out[f"cast_{n}"] = dst
    out.update(_adam(nat, dev, False))
    out.update(_adam(nat, dev, True))
    fam = family(96).to(dev)
    out["sum_chunks"] = nat.sum_chunks(fam.view(1, 96), torch.zeros(96, dtype=torch.bfloat16, device=dev))
    out["column_sums"] = nat.column_sums(fam.view(1, 96), torch.zeros(96, dtype=torch.bfloat16, device=dev))
    out["fold_bias"] = nat.gru_fold_bias(fam, torch.zeros(96, device=dev), torch.bfloat16)[0]       # H = 16

    # ---- computed sites
    cells = 257
    logits = _normal(g, cells, 14, scale=2.0).to(torch.bfloat16).to(dev)
    dense = torch.zeros(cells, 14)
    dense[torch.arange(cells), torch.randint(0, 14, (cells,), generator=g)] = 1.0
    dense = dense.to(dev)
    out["softmax_mse_grad"] = nat.softmax_mse(logits, dense, grad_scale=1.0)[1]
    out["softmax_ce_grad"] = nat.softmax_ce(logits, dense, focal_gamma=2.0, grad_scale=1.0)[1]
    grid = (3, 3)
    frames = 29                                                            # 261 cells
    logits3 = _normal(g, frames, 9, 14, scale=2.0).to(torch.bfloat16).to(dev)
    dense3 = torch.zeros(frames * 9, 14)
    dense3[torch.arange(frames * 9), torch.randint(0, 14, (frames * 9,), generator=g)] = 1.0
    out["smr_loss_grad"] = nat.smr_loss(logits3, dense3.view(frames, 9, 14).to(dev), grid, 1.0, 0.7, 1.3, want_grad=True)[1]

    x = _normal(g, 1, 64, 3, 8).to(torch.bfloat16).to(dev).contiguous(memory_format=torch.channels_last)
    dy = _normal(g, 1, 64, 3, 8).to(torch.bfloat16).to(dev).contiguous(memory_format=torch.channels_last)
    dw = torch.zeros(64, 64, 3, 3, dtype=torch.bfloat16, device=dev).contiguous(memory_format=torch.channels_last)
    out["conv3x3_wgrad_dw"] = nat.conv3x3_wgrad(x, dy, dw).permute(0, 2, 3, 1)          # memory order

    h = 32
    gi_bias, _, w_t = nat.gru_prepare(_normal(g, 6 * h).to(dev), _normal(g, 6 * h).to(dev), _normal(g, 2, 3 * h, h).to(dev),
                                      torch.bfloat16)
    out["prepare_gi_bias"], out["prepare_w_t"] = gi_bias, w_t
    h = 8
    out["dwhh_finish"] = nat.gru_dwhh_finish(_normal(g, 2, 6 * h, 2 * h).to(dev), _normal(g, 2, 2 * h, 2 * h).to(dev),
                                             torch.zeros(2, 3 * h, h, dtype=torch.bfloat16, device=dev))
    torch.cuda.synchronize(dev)
    return out
