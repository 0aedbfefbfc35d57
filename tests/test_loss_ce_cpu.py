"""CPU checks of the cross-entropy class term: the float64 restatement the GPU tests measure against (tests/loss_ce_ref.py)
is pinned to the reference's own numbers (tests/golden/loss_golden.npz), its mask target rule to argmax(mask_to_dense), its
focal gradient to autograd, and the module's CPU path to the fixture."""
import numpy as np
import pytest
import torch

import loss_ce_ref as ref


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(golden_dir / "loss_golden.npz")


def test_restatement_reproduces_the_reference_fixture(golden):
    z = golden
    loss, grad, _ = ref.softmax_ce(z["logits"], z["labels"], z["class_weights"])
    plain, _, w_plain = ref.softmax_ce(z["logits"], z["labels"])
    e_w = abs(loss - float(z["ce_weighted"])) / float(z["ce_weighted"])
    e_u = abs(plain - float(z["ce_unweighted"])) / float(z["ce_unweighted"])
    e_g = np.abs(grad - z["ce_weighted_grad"]).max() / np.abs(z["ce_weighted_grad"]).max()
    print(f"restatement vs fixture: weighted {e_w:.2e}, unweighted {e_u:.2e}, gradient {e_g:.2e} of max")
    assert e_w <= 1e-6 and e_u <= 1e-6 and e_g <= 1e-5
    assert w_plain == z["logits"].size // 14


def test_mask_target_rule_is_argmax_of_mask_to_dense():
    import loss as loss_mod
    masks = [1 << b for b in range(14)]                                   # every single-bit mask
    masks += [0]                                                          # background
    masks += [0b101, 0b110000, (1 << 12) | (1 << 3), 0x1FFF, 0b1010101010]  # multi-hot
    masks += [(1 << 13) | 1, (1 << 13) | (1 << 12), 0x3FFF, (1 << 13) | (1 << 7) | (1 << 2)]   # bit 13 with others
    mask = np.asarray(masks, np.uint16)
    dense = loss_mod.mask_to_dense(torch.from_numpy(mask), 14)
    want = torch.argmax(dense, dim=-1).numpy()
    assert np.array_equal(ref.mask_targets(mask), want)
    assert np.array_equal(ref.targets(dense.numpy()), want)              # the dense rule on the same labels
    assert ref.mask_targets(np.asarray([1 << 13, 0], np.uint16)).tolist() == [13, 13]
    # all 2^14 masks, and bits above the 14 classes are ignored
    every = np.arange(1 << 14, dtype=np.uint16)
    dense = loss_mod.mask_to_dense(torch.from_numpy(every), 14)
    assert np.array_equal(ref.mask_targets(every), torch.argmax(dense, dim=-1).numpy())
    assert np.array_equal(ref.mask_targets(every | np.uint16(0xC000)), ref.mask_targets(every))


def _torch_focal(logits, target, weights, gamma):
    """The definition as a float64 torch expression (autograd gives its gradient)."""
    log_p = torch.log_softmax(logits, dim=-1)
    rows = torch.arange(logits.shape[0])
    log_pt = log_p[rows, target]
    p = log_p.exp()
    keep = torch.ones_like(p)
    keep[rows, target] = 0.0
    q = (p * keep).sum(dim=-1)
    w = weights[target]
    return (w * q.pow(gamma) * -log_pt).sum() / w.sum()


@pytest.mark.parametrize("gamma", [1.0, 2.0])
def test_focal_gradient_of_the_restatement_equals_autograd(gamma):
    g = torch.Generator().manual_seed(int(gamma) + 20)
    n = 3000
    logits = (torch.randn(n, 14, generator=g, dtype=torch.float64) * 3).requires_grad_(True)
    mask = torch.where(torch.rand(n, generator=g) < 0.2, 1 << torch.randint(0, 13, (n,), generator=g),
                       torch.zeros(n, dtype=torch.int64)).to(torch.uint16).numpy()
    weights = (torch.rand(14, generator=g) * 1.95 + 0.05).to(torch.float32)
    target = torch.from_numpy(ref.mask_targets(mask))
    value = _torch_focal(logits, target, weights.double(), gamma)
    value.backward()
    loss, grad, _ = ref.softmax_ce(logits.detach().numpy(), mask, weights.numpy(), gamma)
    e_g = np.abs(grad - logits.grad.numpy()).max() / np.abs(logits.grad.numpy()).max()
    print(f"gamma {gamma}: value {abs(loss - value.item()) / value.item():.2e}, gradient {e_g:.2e} of max")
    assert abs(loss - value.item()) <= 1e-13 * value.item()
    assert e_g <= 1e-12


@pytest.mark.parametrize("gamma", [1.0, 2.0])
def test_module_stock_path_is_the_restatement(gamma):
    """The plain-torch focal expression in loss.py (the GPU tests' torch yardstick) against the restatement, fp32."""
    import loss as loss_mod
    g = torch.Generator().manual_seed(31)
    logits = (torch.randn(2, 5, 648, 14, generator=g) * 2).requires_grad_(True)
    mask = ((torch.rand(2, 5, 648, generator=g) < 0.1).to(torch.int32) << 4).to(torch.uint16)
    weights = torch.ones(14)
    weights[13] = 0.05
    crit = loss_mod.SMRSELDLoss("ce", class_weights=weights, focal_gamma=gamma)
    total, breakdown = crit(logits, mask)
    total.backward()
    loss, grad, _ = ref.softmax_ce(logits.detach().numpy(), mask.numpy(), weights.numpy(), gamma)
    assert set(breakdown) == {"class_ce"}
    assert abs(total.item() - loss) <= 1e-5 * loss
    assert np.abs(logits.grad.numpy() - grad).max() <= 1e-4 * np.abs(grad).max()


def test_module_on_the_cpu_still_returns_the_fixture(golden):
    import loss as loss_mod
    z = golden
    crit = loss_mod.SMRSELDLoss("ce", class_weights=torch.from_numpy(z["class_weights"]), focal_gamma=0)
    total, breakdown = crit(torch.from_numpy(z["logits"]), torch.from_numpy(z["labels"]))
    assert abs(total.item() - float(z["ce_weighted"])) <= 1e-6 * float(z["ce_weighted"])
    assert abs(breakdown["class_ce"] - float(z["ce_weighted"])) <= 1e-6 * float(z["ce_weighted"])
    plain = loss_mod.SMRSELDLoss("ce")
    assert plain.focal_gamma == 0.0
    assert abs(plain(torch.from_numpy(z["logits"]), torch.from_numpy(z["labels"]))[0].item()
               - float(z["ce_unweighted"])) <= 1e-6 * float(z["ce_unweighted"])


@pytest.mark.parametrize("gamma", [-1.0, 0.5, 0.999, float("inf"), float("nan")])
def test_module_refuses_gamma_outside_zero_or_at_least_one(gamma):
    import loss as loss_mod
    with pytest.raises(ValueError, match="focal_gamma"):
        loss_mod.SMRSELDLoss("ce", focal_gamma=gamma)


def test_config_default_and_trainer_hand_over():
    import inspect
    import config
    import trainer
    assert config.Config.CE_FOCAL_GAMMA == 0.0
    assert inspect.getsource(trainer).count('focal_gamma=getattr(config, "CE_FOCAL_GAMMA", 0.0)') == 2
