"""GPU parity of the fused cross-entropy class loss (csrc/loss_ce.hip; loss.py:27-41 plus the optional focal factor) against
the reference's own numbers (tests/golden/loss_golden.npz), the float64 restatement tests/loss_ce_ref.py (pinned to that
fixture and to autograd by tests/test_loss_ce_cpu.py) and the module's stock torch path."""
import ctypes

import numpy as np
import pytest
import torch

import loss_ce_ref as ref
from oracle import labels as olab

pytestmark = pytest.mark.gpu


def _weights(device, generator):
    return (torch.rand(14, generator=generator) * 1.95 + 0.05).to(device)          # random in [0.05, 2]


def test_matches_reference_loss_golden(gpu_device, golden_dir):
    import seld_native
    z = np.load(golden_dir / "loss_golden.npz")
    logits = torch.from_numpy(z["logits"]).to(gpu_device)
    labels = torch.from_numpy(z["labels"]).to(gpu_device)
    weights = torch.from_numpy(z["class_weights"]).to(gpu_device)
    loss, grad = seld_native.softmax_ce(logits, labels, weights, grad_scale=1.0)
    want, want_grad = float(z["ce_weighted"]), z["ce_weighted_grad"]
    err_g = np.abs(grad.cpu().numpy() - want_grad).max() / np.abs(want_grad).max()
    print(f"weighted: {loss.item():.7f} vs {want:.7f}; gradient {err_g:.2e} of max")
    assert abs(loss.item() - want) <= 1e-5 * abs(want)
    assert err_g <= 1e-3
    plain, none = seld_native.softmax_ce(logits, labels)
    assert none is None and abs(plain.item() - float(z["ce_unweighted"])) <= 1e-5 * float(z["ce_unweighted"])
    loss2, grad2 = seld_native.softmax_ce(logits, labels, weights, grad_scale=1.0)
    assert loss2.item() == loss.item() and torch.equal(grad2, grad)                 # deterministic


@pytest.mark.parametrize("gamma", [0.0, 2.0])
def test_mask_labels_equal_dense_labels(gpu_device, gamma):
    import loss as loss_mod
    import seld_native
    g = torch.Generator().manual_seed(3)
    B, T = 3, 250
    logits = (torch.randn(B, T, 648, 14, generator=g) * 3).to(gpu_device)
    mask_np = olab.metadata_to_mask(olab.synth_metadata(5, 150), 750 * 480)[:750].reshape(B, T, 648).copy()
    flat = mask_np.reshape(-1)
    flat[[5, 700, 70000, 300001]] = [0b101, (1 << 13) | 1, (1 << 13) | (1 << 12) | (1 << 6), 0x3FFF]   # multi-hot cells
    flat[-1] = 1 << 13                                                  # the background bit alone
    mask = torch.from_numpy(mask_np).to(gpu_device)
    dense = loss_mod.mask_to_dense(mask, 14)
    weights = _weights(gpu_device, g)
    l1, g1, w1 = seld_native.softmax_ce(logits, mask, weights, gamma, grad_scale=1.0, return_weight_sum=True)
    l2, g2, w2 = seld_native.softmax_ce(logits, dense, weights, gamma, grad_scale=1.0, return_weight_sum=True)
    assert l1.item() == l2.item() and w1.item() == w2.item() and torch.equal(g1, g2)
    assert int((mask != 0).sum()) > 100 and np.isfinite(l1.item())


RAGGED = [1, 255, 256, 257, 648 * 7 + 2, 2048 * 256 + 1]
_ragged_inputs = {}


def _ragged(n_cells, device):
    """Logits, labels, weights and the float64 references of one size: built once, shared by both gamma cases."""
    if n_cells not in _ragged_inputs:
        g = torch.Generator().manual_seed(n_cells)
        logits = torch.randn(n_cells, 14, generator=g) * 2
        cls = torch.randint(0, 13, (n_cells,), generator=g)
        mask = torch.where(torch.rand(n_cells, generator=g) < 0.05, 1 << cls, torch.zeros_like(cls))
        mask = mask | torch.where(torch.rand(n_cells, generator=g) < 0.01, 1 << 5, 0)       # a few second classes
        mask = mask.to(torch.uint16)
        weights = torch.rand(14, generator=g) * 1.95 + 0.05
        seen = {torch.float32: logits, torch.bfloat16: logits.to(torch.bfloat16)}
        refs = {(dt, gamma): ref.softmax_ce(lg.float().numpy(), mask.numpy(), weights.numpy(), gamma)
                for dt, lg in seen.items() for gamma in (0.0, 2.0)}
        import loss as loss_mod
        _ragged_inputs[n_cells] = ({dt: lg.to(device) for dt, lg in seen.items()}, mask.to(device),
                                   loss_mod.mask_to_dense(mask, 14).to(device), weights.to(device), refs)
    return _ragged_inputs[n_cells]


@pytest.mark.parametrize("gamma", [0.0, 2.0])
@pytest.mark.parametrize("n_cells", RAGGED)
def test_every_instantiation_at_ragged_sizes(gpu_device, n_cells, gamma):
    """fp32 / bf16 logits x mask / dense labels x value-only / value + gradient x plain / focal, at sizes whose last tile is
    ragged (and one at which a block walks more than one tile), against the float64 restatement on the logits as the kernel
    sees them (the bf16 values cast up)."""
    import seld_native
    logits, mask, dense, weights, refs = _ragged(n_cells, gpu_device)
    for dtype in (torch.float32, torch.bfloat16):
        want, want_grad, want_w = refs[(dtype, gamma)]
        g_max = np.abs(want_grad).max()
        for labels in (mask, dense):
            value, none, w_sum = seld_native.softmax_ce(logits[dtype], labels, weights, gamma, return_weight_sum=True)
            value2, grad = seld_native.softmax_ce(logits[dtype], labels, weights, gamma, grad_scale=1.0)
            err_g = np.abs(grad.float().cpu().numpy().astype(np.float64) - want_grad).max() / g_max
            print(f"n {n_cells} gamma {gamma} {dtype} {labels.dtype}: value {abs(value.item() - want) / want:.2e} "
                  f"gradient {err_g:.2e} of max, W {abs(w_sum.item() - want_w) / want_w:.2e}")
            assert none is None and grad.dtype == dtype and grad.shape == logits[dtype].shape
            assert value.item() == value2.item()
            assert abs(value.item() - want) <= 1e-5 * want
            assert abs(w_sum.item() - want_w) <= 1e-7 * want_w
            assert err_g <= (1e-4 if dtype == torch.float32 else 8e-3)


@pytest.mark.parametrize("gamma", [0.0, 2.0])
def test_edge_cases(gpu_device, gamma):
    import seld_native
    g = torch.Generator().manual_seed(17)
    n = 600
    logits = torch.randn(n, 14, generator=g) * 2
    mask = torch.where(torch.rand(n, generator=g) < 0.3, 1 << torch.randint(0, 13, (n,), generator=g), 0).to(torch.uint16)
    # the target logit dominates by 60: p_t rounds to 1 and log p_t to 0, the focal factor q^2 ~ 1e-50 is below fp32
    logits[3] = -30.0
    logits[3, 4] = 30.0
    mask[3] = 1 << 4
    # ... and by 120: every other exponential underflows, q == 0 exactly, the branch that contributes nothing
    logits[4] = -60.0
    logits[4, 13] = 60.0
    mask[4] = 0
    # +-80 in one cell, the target at -80: only the subtraction of the maximum keeps exp and log p_t = -160 finite
    logits[5, :7] = 80.0
    logits[5, 7:] = -80.0
    mask[5] = 1 << 9
    weights = torch.rand(14, generator=g) * 1.95 + 0.05
    weights[2] = 0.0                                       # a class that occurs, with weight zero: out of value, gradient and W
    mask[6] = 1 << 2
    for lab, w in ((mask, weights), (torch.zeros(n, dtype=torch.uint16), weights)):      # second: a batch that is all background
        want, want_grad, want_w = ref.softmax_ce(logits.numpy(), lab.numpy(), w.numpy(), gamma)
        value, grad, w_sum = seld_native.softmax_ce(logits.to(gpu_device), lab.to(gpu_device), w.to(gpu_device), gamma,
                                                    grad_scale=1.0, return_weight_sum=True)
        got = grad.cpu().numpy()
        assert np.isfinite(value.item()) and np.isfinite(got).all()
        assert abs(value.item() - want) <= 1e-5 * want and abs(w_sum.item() - want_w) <= 1e-7 * want_w
        assert np.abs(got - want_grad).max() <= 1e-4 * np.abs(want_grad).max()
        if lab is mask:
            assert not got[6].any()                        # weight zero
            assert not got[4].any()                        # q == 0
            if gamma:
                assert not got[3].any()                    # q^gamma underflows
        else:
            assert abs(want_w - n * float(w[13])) <= 1e-12 * want_w


@pytest.mark.parametrize("gamma", [0.0, 2.0])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_module_backward_with_and_without_upstream_scale(gpu_device, dtype, gamma):
    """SMRSELDLoss('ce') through autograd, fused against the same module with fused_enabled = False: loss.backward()
    (upstream gradient exactly 1) and (0.37 * loss).backward() (scaled in place by the device scalar)."""
    import loss as loss_mod
    g = torch.Generator().manual_seed(9)
    logits = (torch.randn(2, 30, 648, 14, generator=g) * 2).to(gpu_device).to(dtype)
    mask = torch.randint(0, 1 << 13, (2, 30, 648), generator=g).to(torch.uint16).to(gpu_device)
    weights = torch.ones(14, device=gpu_device)
    weights[13] = 0.05
    crit = loss_mod.SMRSELDLoss("ce", 1.0, grid_size=(18, 36), class_weights=weights, focal_gamma=gamma)
    saved = loss_mod.SMRSELDLoss.fused_enabled
    try:
        for factor in (1.0, 0.37):
            results = {}
            for fused in (True, False):
                loss_mod.SMRSELDLoss.fused_enabled = fused
                a = logits.clone().requires_grad_(True)
                total, term = crit.loss_tensor(a, mask)
                (total * factor if factor != 1.0 else total).backward()
                results[fused] = (total.item(), a.grad.float())
            (v_f, g_f), (v_s, g_s) = results[True], results[False]
            tol = 1e-4 if dtype == torch.float32 else 1e-2
            assert abs(v_f - v_s) <= 1e-5 * v_s, (factor, v_f, v_s)
            assert (g_f - g_s).abs().max().item() <= tol * g_s.abs().max().item(), factor
    finally:
        loss_mod.SMRSELDLoss.fused_enabled = saved


def test_ce_trains_through_the_captured_step(gpu_device):
    """LOSS_TYPE 'ce' with the trainer's class weights on the full-size CRNN, bf16 master weights, captured iterations."""
    import dataset
    import loss as loss_mod
    import trainer
    from oracle import features as ofeat
    cfg = trainer.config
    saved = (cfg.MODEL_TYPE, cfg.SEED, loss_mod.SMRSELDLoss.fused_enabled)
    cfg.MODEL_TYPE, cfg.SEED = "crnn", 3
    steppers = []
    try:
        clips = [ofeat.synth_pcm(i, 4, 24000 * 8, "noise") for i in range(2)]
        rows = [olab.synth_metadata(i, meta_frames=80) for i in range(2)]
        ds = dataset.SELDDataset.from_pcm(clips, rows, device=gpu_device)
        weights = torch.ones(cfg.NUM_CLASSES, device=gpu_device)
        weights[cfg.NUM_CLASSES - 1] = 0.05

        def make():
            torch.manual_seed(0)
            model = trainer.prepare_model_for_device(trainer.build_model((ds.I, ds.J)), gpu_device).train()
            trainer.enable_master_weights(model, gpu_device)
            crit = loss_mod.SMRSELDLoss("ce", 1.0, grid_size=(ds.I, ds.J), class_weights=weights)
            opt = trainer.make_optimizer(model, 1e-3, gpu_device, capturable=trainer.graph_step_enabled(gpu_device))
            steppers.append(trainer.make_stepper(model, crit, opt, gpu_device))
            return model, crit, steppers[-1]

        spec, mask = ds.device_batch([0, 3])
        model, crit, step = make()
        assert loss_mod.SMRSELDLoss.fused_enabled
        torch.manual_seed(11)                                         # the dropout masks of the first iteration
        losses = []
        for _ in range(6):
            total, term = step(spec, mask)
            losses.append(total.item())
        assert all(np.isfinite(losses)) and losses[-1] < losses[0], losses
        if hasattr(step, "stats"):
            assert step.stats()["graphs"] >= 1 and step.stats()["capture_error"] is None, step.stats()
        with torch.no_grad(), trainer.autocast_context(gpu_device):
            total, breakdown = crit(model.eval()(spec), mask)
        assert set(breakdown) == {"class_ce"}
        # the stock path on the same initial weights and the same dropout masks
        _, _, stock_step = make()
        loss_mod.SMRSELDLoss.fused_enabled = False
        torch.manual_seed(11)
        stock = stock_step(spec, mask)[0].item()
        print(f"captured 'ce' step: losses {losses}; stock first loss {stock}")
        assert abs(losses[0] - stock) <= 1e-3 * stock
    finally:
        for s in steppers:
            if hasattr(s, "close"):
                s.close()
        cfg.MODEL_TYPE, cfg.SEED, loss_mod.SMRSELDLoss.fused_enabled = saved


# ---- what the entry point refuses, through the C ABI --------------------------------------------------------------------

INVALID, UNSUPPORTED = -1, -4
LIMIT = (2147483647 - 4096) // 14                  # the largest n_cells seld_softmax_mse accepts
REFUSALS = [("num_classes = 13", {"num_classes": 13}, UNSUPPORTED), ("num_classes = 15", {"num_classes": 15}, UNSUPPORTED),
            ("n_cells = 0", {"n_cells": 0}, INVALID), ("n_cells = -1", {"n_cells": -1}, INVALID),
            ("n_cells * 14 at the limit", {"n_cells": LIMIT + 1}, UNSUPPORTED),
            ("null logits", {"logits": None}, INVALID), ("null out", {"out": None}, INVALID),
            ("null workspace", {"workspace": None}, INVALID),
            ("mask and dense labels", {"dense": "dense"}, INVALID), ("neither mask nor dense labels", {"mask": None}, INVALID),
            ("gamma = -1", {"gamma": -1.0}, INVALID), ("gamma = 0.5", {"gamma": 0.5}, INVALID),
            ("gamma = 0.999", {"gamma": 0.999}, INVALID), ("gamma = inf", {"gamma": float("inf")}, INVALID),
            ("gamma = nan", {"gamma": float("nan")}, INVALID)]


@pytest.fixture(scope="module")
def entry(gpu_device):
    import seld_native
    seld_native.ensure_init(gpu_device)
    lib = seld_native.load_library()
    n = 300
    bufs = {"logits": torch.randn(n, 14, device=gpu_device), "mask": torch.zeros(n, dtype=torch.uint16, device=gpu_device),
            "dense": torch.zeros(n, 14, device=gpu_device), "weights": torch.ones(14, device=gpu_device),
            "out": torch.full((2,), 77.0, device=gpu_device), "grad": torch.full((n, 14), 77.0, device=gpu_device),
            "workspace": torch.full((lib.seld_softmax_ce_workspace_bytes(),), 77, dtype=torch.uint8, device=gpu_device)}
    yield lib, bufs, n, seld_native._stream_ptr(gpu_device)


@pytest.mark.parametrize("case,overrides,expected", REFUSALS, ids=[c[0] for c in REFUSALS])
def test_entry_point_refuses(entry, case, overrides, expected):
    lib, bufs, n, stream = entry
    a = {"logits": "logits", "mask": "mask", "dense": None, "n_cells": n, "num_classes": 14, "gamma": 0.0, "out": "out",
         "workspace": "workspace"}
    a.update(overrides)

    def p(name):
        return ctypes.c_void_p(bufs[a[name]].data_ptr()) if a[name] is not None else None

    rc = lib.seld_softmax_ce(p("logits"), 0, p("mask"), p("dense"), a["n_cells"], a["num_classes"],
                             ctypes.c_void_p(bufs["weights"].data_ptr()), a["gamma"], 1.0, p("out"),
                             ctypes.c_void_p(bufs["grad"].data_ptr()), p("workspace"), stream)
    print(case, rc, lib.seld_last_error())
    assert rc == expected and lib.seld_last_error().startswith(b"seld_softmax_ce:")
    torch.cuda.synchronize()
    assert bool((bufs["out"] == 77.0).all()) and bool((bufs["grad"] == 77.0).all()) and bool((bufs["workspace"] == 77).all())


def test_python_entry_refuses_gamma_between_zero_and_one(gpu_device):
    import seld_native
    logits = torch.randn(10, 14, device=gpu_device)
    mask = torch.zeros(10, dtype=torch.uint16, device=gpu_device)
    with pytest.raises(seld_native.SeldNativeError):
        seld_native.softmax_ce(logits, mask, focal_gamma=0.5)
