"""GPU tests of the first encoder block with its convolution recomputed in place (csrc/convfirst.hip,
seld_native.convfirst_forward / convfirst_backward, seld_convfirst).

Reference: the stock Conv2d -> BatchNorm2d -> ReLU -> MaxPool2d((1, 2)) in fp32 on the same bf16-rounded input and
weights.  Against it stand today's general path (the library's bf16 convolution, seld_native.conv_tail_forward /
conv_tail_backward, aten.convolution_backward) and the new kernels.  The two differ only in the order in which the 36
products of an output are added ahead of the same single rounding to bf16, so their errors against the reference must be
equal statistically: no absolute tolerance, the new error is held to a multiple of the old one.

Element-wise parity (every y bit for bit, every dW element under a derived bound, edges, the chunk walk, guard regions)
is in tests/test_convfirst_parity_gpu.py."""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

CL = torch.channels_last
FP32_ULPS = 8 * 2.0 ** -24          # floor for quantities whose two errors are both fp32 rounding noise (relative L2)


def _case(b, t, f, device, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    x = (torch.randn(b, 4, t, f, generator=g) * 20 - 30).to(device=device, dtype=torch.bfloat16).contiguous(memory_format=CL)
    torch.manual_seed(seed)
    conv = nn.Conv2d(4, 64, 3, padding=1, bias=False)
    w = conv.weight.detach().to(device=device, dtype=torch.bfloat16).contiguous(memory_format=CL)
    gamma = (1.0 + 0.2 * torch.randn(64, generator=g)).to(device)
    beta = (0.1 * torch.randn(64, generator=g)).to(device)
    go = torch.randn(b, 64, t, f // 2, generator=g).to(device=device, dtype=torch.bfloat16).contiguous(memory_format=CL)
    return x, w, gamma, beta, go


def _reference(x, w, gamma, beta, go):
    """fp32 stock modules on the bf16-rounded operands"""
    w32 = w.float().clone().requires_grad_(True)
    bn = nn.BatchNorm2d(64).to(x.device).train()
    with torch.no_grad():
        bn.weight.copy_(gamma)
        bn.bias.copy_(beta)
    y = F.max_pool2d(F.relu(bn(F.conv2d(x.float(), w32, padding=1))), (1, 2))
    y.backward(go.float())
    return dict(y=y.detach(), dw=w32.grad, dgamma=bn.weight.grad, dbeta=bn.bias.grad, running_mean=bn.running_mean,
                running_var=bn.running_var)


def _general_path(x, w, gamma, beta, go):
    """what the block runs without the first-block kernels"""
    import seld_native
    rm, rv = torch.zeros(64, device=x.device), torch.ones(64, device=x.device)
    x1 = F.conv2d(x, w, padding=1)
    y, mean_invstd, scale_shift = seld_native.conv_tail_forward(x1, gamma, beta, rm, rv, 0.1, 1e-5, True, 2)
    dx1, dgamma, dbeta = seld_native.conv_tail_backward(x1, go, mean_invstd, scale_shift, 2)
    dw = torch.ops.aten.convolution_backward(dx1, x, w, None, (1, 1), (1, 1), (1, 1), False, (0, 0), 1,
                                             (False, True, False))[1]
    return dict(y=y, dw=dw, dgamma=dgamma, dbeta=dbeta, running_mean=rm, running_var=rv)


def _new_path(x, w, gamma, beta, go, dw_dtype=torch.bfloat16):
    import seld_native
    rm, rv = torch.zeros(64, device=x.device), torch.ones(64, device=x.device)
    y, mean_invstd, scale_shift = seld_native.convfirst_forward(x, w, gamma, beta, rm, rv, 0.1, 1e-5)
    dw = torch.empty(64, 4, 3, 3, dtype=dw_dtype, device=x.device).contiguous(memory_format=CL)
    dw, dgamma, dbeta = seld_native.convfirst_backward(x, w, go, mean_invstd, scale_shift, dw)
    return dict(y=y, dw=dw, dgamma=dgamma, dbeta=dbeta, running_mean=rm, running_var=rv, mean_invstd=mean_invstd,
                scale_shift=scale_shift)


def _rel(got, want):
    return (got.float() - want).norm().item() / max(want.norm().item(), 1e-30)


# the bench's shape (ratio 1.25: 32.8 M samples), a ragged one (odd B, T not a multiple of the rows per chunk) and a
# second legal F, plus a single short clip at the widest F (ratio 2: a few thousand samples make the ratio itself noisy)
@pytest.mark.parametrize("b,t,f,factor", [(32, 250, 64, 1.25), (3, 11, 64, 2.0), (2, 37, 32, 2.0), (1, 3, 256, 2.0),
                                          (5, 9, 16, 2.0)])
def test_errors_against_fp32_reference_match_the_general_path(gpu_device, b, t, f, factor):
    import seld_native
    x, w, gamma, beta, go = _case(b, t, f, gpu_device, seed=100 * b + t + f)
    assert seld_native.convfirst_applicable(x, w)
    ref = _reference(x, w, gamma, beta, go)
    old = _general_path(x, w, gamma, beta, go)
    new = _new_path(x, w, gamma, beta, go)
    torch.cuda.synchronize()
    assert new["y"].dtype == torch.bfloat16 and new["y"].shape == ref["y"].shape
    assert new["y"].is_contiguous(memory_format=CL)
    report, failures = [], []
    for name in ("y", "dw", "dgamma", "dbeta", "running_mean", "running_var"):
        e_old, e_new = _rel(old[name], ref[name]), _rel(new[name], ref[name])
        floor = FP32_ULPS if name.startswith("running") else 0.0
        report.append(f"{name}: general {e_old:.3e}  first-block {e_new:.3e}")
        if not e_new <= factor * e_old + floor:
            failures.append(name)
    print(f"\n(B, T, F) = ({b}, {t}, {f}) relative L2 against the fp32 reference\n  " + "\n  ".join(report))
    assert not failures, (failures, report)


def test_fp32_weight_and_fp32_gradient(gpu_device):
    """fp32 parameters (no master-weight mode): the kernels round the weight like autocast's cast and write an fp32
    gradient whose bf16 rounding is the bf16 gradient; standard (not channels-last) weight strides are honoured."""
    import seld_native
    x, w, gamma, beta, go = _case(3, 11, 64, gpu_device, seed=5)
    w32 = w.float().contiguous()                                  # standard strides, exactly representable in bf16
    a = _new_path(x, w, gamma, beta, go, torch.float32)
    rm, rv = torch.zeros(64, device=gpu_device), torch.ones(64, device=gpu_device)
    y, mean_invstd, scale_shift = seld_native.convfirst_forward(x, w32, gamma, beta, rm, rv, 0.1, 1e-5)
    dw = torch.empty_like(w32)
    seld_native.convfirst_backward(x, w32, go, mean_invstd, scale_shift, dw)
    b16 = _new_path(x, w, gamma, beta, go, torch.bfloat16)
    torch.cuda.synchronize()
    assert torch.equal(y, a["y"]) and torch.equal(rm, a["running_mean"]) and torch.equal(rv, a["running_var"])
    assert torch.equal(dw, a["dw"]) and not dw.is_contiguous(memory_format=CL)
    assert torch.equal(a["dw"].to(torch.bfloat16), b16["dw"])


@pytest.mark.parametrize("b,t,f", [(32, 250, 64), (3, 11, 64)])
def test_two_calls_are_bit_identical(gpu_device, b, t, f):
    x, w, gamma, beta, go = _case(b, t, f, gpu_device, seed=9)
    one = _new_path(x, w, gamma, beta, go)
    two = _new_path(x, w, gamma, beta, go)
    torch.cuda.synchronize()
    for name, value in one.items():
        assert torch.equal(value, two[name]), name


def test_convblock_dispatch_and_gating(gpu_device):
    """ConvBlock takes the first-block path only in the bf16 training configuration; its switch, the tail's switch, eval
    mode, an fp32 input and an input that needs a gradient all keep the general path."""
    import seld_convfirst
    import seld_convtail
    import seld_native
    from model_crnn import ConvBlock
    calls = []
    real = seld_native.convfirst_forward

    def counted(*args, **kw):
        calls.append(1)
        return real(*args, **kw)
    seld_native.convfirst_forward = counted
    try:
        torch.manual_seed(3)
        block = ConvBlock(4, 64, pool_size=(1, 2)).to(gpu_device).to(memory_format=CL).train()
        x = (torch.randn(3, 4, 20, 64, device=gpu_device) * 20 - 30).to(torch.bfloat16).contiguous(memory_format=CL)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            y = block(x)
            assert len(calls) == 1 and y.dtype == torch.bfloat16
            y.float().square().mean().backward()
            grads = [p.grad for p in block.parameters()]
            assert all(g is not None and torch.isfinite(g).all() for g in grads)
            assert block.bn.num_batches_tracked.item() == 1
            seld_convfirst.enabled = False
            try:
                y_general = block(x)
            finally:
                seld_convfirst.enabled = True
            assert len(calls) == 1
            assert _rel(y, y_general.float()) <= 2e-2
            seld_convtail.enabled = False
            try:
                block(x)
            finally:
                seld_convtail.enabled = True
            assert len(calls) == 1
            block(x.detach().requires_grad_(True))
            block(x.float())
            with torch.no_grad():
                block(x)
            block.eval()
            block(x)
            assert len(calls) == 1
            wide = ConvBlock(36, 64, pool_size=(1, 2)).to(gpu_device).to(memory_format=CL).train()
            wide(torch.randn(2, 36, 5, 64, device=gpu_device).to(torch.bfloat16).contiguous(memory_format=CL))
            assert len(calls) == 1
    finally:
        seld_native.convfirst_forward = real


def test_captured_step_runs_the_first_block_kernels(gpu_device):
    """The bench's configuration (seld_graph.GraphedTrainStep, master weights): the first-block entry points run once per
    step, forward and backward, in the eager warm-up steps and in the capture; with the switch off they do not run and
    the replayed losses track the fused run (the two differ by a summation order ahead of a bf16 rounding, like the
    weight-gradient kernel of blocks 2-4 in test_conv_wgrad_gpu.py, whose bound this is)."""
    import seld_convfirst
    import seld_graph
    import seld_native
    import trainer
    import model_crnn
    calls = {"forward": 0, "backward": 0}
    real_f, real_b = seld_native.convfirst_forward, seld_native.convfirst_backward

    def counted_f(*args, **kw):
        calls["forward"] += 1
        return real_f(*args, **kw)

    def counted_b(*args, **kw):
        calls["backward"] += 1
        return real_b(*args, **kw)

    g = torch.Generator().manual_seed(5)
    batches = [((torch.randn(4, 250, 4, 64, generator=g) * 20 - 30).to(gpu_device),
                ((torch.rand(4, 250, 648, generator=g) < 0.02).to(torch.int32) << 3).to(torch.uint16).to(gpu_device))
               for _ in range(6)]

    def run(fused):
        try:
            torch.manual_seed(0)
            model = trainer.prepare_model_for_device(model_crnn.SELD_CRNN(), gpu_device).train()
            for m in model.modules():
                if isinstance(m, torch.nn.Dropout):
                    m.p = 0.0
            model.rnn.dropout = 0.0
            seld_convfirst.enabled = fused                    # (prepare_model_for_device sets it from the config)
            seld_native.convfirst_forward, seld_native.convfirst_backward = counted_f, counted_b
            trainer.enable_master_weights(model, gpu_device)
            crit = trainer.SMRSELDLoss("mse", 1.0, grid_size=(18, 36))
            opt = trainer.make_optimizer(model, 1e-3, gpu_device, capturable=True)
            step = seld_graph.GraphedTrainStep(model, crit, opt, gpu_device,
                                               autocast=lambda: trainer.autocast_context(gpu_device), use_graphs=True)
            losses = torch.stack([step(x, m)[0].clone() for x, m in batches]).cpu()
            captured = step.stats().get("capture_error")
            step.close()
            return losses, captured
        finally:
            seld_native.convfirst_forward, seld_native.convfirst_backward = real_f, real_b
            seld_convfirst.enabled = True

    on, on_err = run(True)
    assert on_err is None, on_err
    assert calls["forward"] >= 4 and calls["forward"] == calls["backward"], calls      # 3 eager steps + the capture
    seen = dict(calls)
    off, off_err = run(False)
    assert off_err is None, off_err
    assert calls == seen, (calls, seen)
    rel = ((on - off).abs() / off.abs()).max().item()
    print("\nlosses, first-block kernels on / off:", on.tolist(), off.tolist(), "max relative difference", rel)
    assert rel <= 5e-3, (on, off)
