"""GPU parity of the 3x3-convolution weight gradient (csrc/convwgrad.hip, seld_native.conv3x3_wgrad) that
model_crnn._Conv3x3.backward uses for the encoder's blocks 2-4.

Reference: aten.convolution_backward in fp32 on the same bf16-rounded inputs.  Both sides accumulate in fp32 in
different orders, so the bar is an fp32 accumulation error (a small multiple of eps times the sum of |terms|,
computed as the same product of |dy| and |x|) plus, for a bf16 gradient, one bf16 rounding (2^-8 relative).
"""
import pytest
import torch

pytestmark = pytest.mark.gpu


def _case(b, cin, cout, t, f, device, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    x = torch.randn(b, cin, t, f, generator=g).to(device=device, dtype=torch.bfloat16)
    dy = (torch.randn(b, cout, t, f, generator=g) * 0.1).to(device=device, dtype=torch.bfloat16)
    cl = torch.channels_last
    return x.contiguous(memory_format=cl), dy.contiguous(memory_format=cl)


def _reference(x, dy, cin):
    w = torch.empty(dy.shape[1], cin, 3, 3, device=x.device)
    args = ((1, 1), (1, 1), (1, 1), False, (0, 0), 1, (False, True, False))
    ref = torch.ops.aten.convolution_backward(dy.float(), x.float(), w, None, *args)[1]
    mag = torch.ops.aten.convolution_backward(dy.float().abs(), x.float().abs(), w, None, *args)[1]
    return ref, mag


def _dw(cout, cin, dtype, device):
    return torch.empty(cout, cin, 3, 3, dtype=dtype, device=device, memory_format=torch.channels_last)


# the encoder's blocks 2-4 at the bench batch (B = 32, T = 250), and ragged cases: odd B, T not a multiple of the
# time rows per chunk (16 / 8 / 4 at F = 8 / 16 / 32), a single clip shorter than one chunk, and a last K slab shorter
# than the others (B = 31 at 64->128, F = 32: 1953 chunks, 8 per slab, the 245th slab holds one)
@pytest.mark.parametrize("b,cin,cout,t,f", [(32, 64, 128, 250, 32), (32, 128, 256, 250, 16), (32, 256, 512, 250, 8),
                                            (3, 64, 64, 37, 8), (5, 128, 64, 13, 16), (1, 64, 192, 3, 32),
                                            (31, 64, 128, 250, 32)])
def test_matches_convolution_backward(gpu_device, b, cin, cout, t, f):
    import seld_native
    x, dy = _case(b, cin, cout, t, f, gpu_device, seed=b * 1000 + cin + f)
    assert seld_native.conv3x3_wgrad_applicable(x, dy, _dw(cout, cin, torch.bfloat16, gpu_device))
    ref, mag = _reference(x, dy, cin)
    for dtype, rounding in ((torch.float32, 0.0), (torch.bfloat16, 2.0 ** -8)):
        dw = seld_native.conv3x3_wgrad(x, dy, _dw(cout, cin, dtype, gpu_device))
        torch.cuda.synchronize()
        err = (dw.float() - ref).abs()
        bound = 1e-5 * mag + rounding * ref.abs() + 1e-30
        worst = (err / bound).max().item()
        assert worst <= 1.0, (dtype, worst, err.max().item(), ref.abs().max().item())


def test_two_calls_are_bit_identical(gpu_device):
    import seld_native
    x, dy = _case(32, 256, 512, 250, 8, gpu_device, seed=7)
    for dtype in (torch.bfloat16, torch.float32):
        a = seld_native.conv3x3_wgrad(x, dy, _dw(512, 256, dtype, gpu_device))
        b = seld_native.conv3x3_wgrad(x, dy, _dw(512, 256, dtype, gpu_device))
        torch.cuda.synchronize()
        assert torch.equal(a, b), dtype


def _crnn_two_steps(device, fused):
    """Two eager master-weight training steps of the full-size CRNN (bf16 working weights, fp32 masters; the weight
    gradients on the main stream: the side stream is the captured step's, see the next test); returns both losses, the
    first step's conv weight gradients and the input channel counts of the weight gradients the HIP kernel computed."""
    import model_crnn
    import seld_native
    import trainer
    from loss import SMRSELDLoss
    calls = []
    real = seld_native.conv3x3_wgrad

    def counted(x, dy, dw):
        calls.append(x.shape[1])
        return real(x, dy, dw)
    was = model_crnn._Conv3x3.fused_wgrad
    try:
        torch.manual_seed(1234)
        model = trainer.prepare_model_for_device(model_crnn.SELD_CRNN(), device).train()
        model_crnn._Conv3x3.fused_wgrad = fused            # (prepare_model_for_device sets it from the config)
        seld_native.conv3x3_wgrad = counted
        model.rnn.dropout = 0.0
        model.fnn[3].p = 0.0
        crit = SMRSELDLoss("mse", 1.0, grid_size=(18, 36))
        trainer.enable_master_weights(model, device)
        opt = trainer.make_optimizer(model, 1e-3, device)
        g = torch.Generator().manual_seed(99)
        x = (torch.randn(4, 250, 4, 64, generator=g) * 20 - 30).to(device)
        mask = ((torch.rand(4, 250, 648, generator=g) < 0.02).to(torch.int32)
                << torch.randint(0, 13, (4, 250, 648), generator=g).to(torch.int32)).to(torch.uint16).to(device)
        losses, grads = [], None
        for _ in range(2):
            opt.zero_grad(set_to_none=True)
            with trainer.autocast_context(device):
                logits = model(x)
            loss, _ = crit.loss_tensor(logits, mask)
            loss.backward()
            if grads is None:
                torch.cuda.synchronize()
                grads = {k: p.grad.detach().float().clone() for k, p in model.named_parameters()
                         if k.endswith("conv.weight")}
            opt.step()
            losses.append(loss.item())
        torch.cuda.synchronize()
        return losses, grads, calls
    finally:
        seld_native.conv3x3_wgrad = real
        model_crnn._Conv3x3.fused_wgrad = was


def test_crnn_training_step_with_and_without_the_kernel(gpu_device):
    on_losses, on_grads, on_calls = _crnn_two_steps(gpu_device, True)
    off_losses, off_grads, off_calls = _crnn_two_steps(gpu_device, False)
    assert sorted(on_calls) == [64, 64, 128, 128, 256, 256], on_calls      # blocks 2-4, two steps
    assert off_calls == []
    # the same forward (two model builds: the library's forward solvers need not give the same bits twice)
    assert abs(on_losses[0] - off_losses[0]) <= 1e-5 * off_losses[0], (on_losses, off_losses)
    assert abs(on_losses[1] - off_losses[1]) <= 5e-3 * off_losses[1], (on_losses, off_losses)
    # bf16 gradients: the library's own weight gradients (block 1 in both runs, blocks 2-4 in the second) add with
    # atomics in a varying order, and that alone moves block 1's bf16 gradient by 1-2 % (relative L2) between two runs;
    # a wrong tap or channel mapping would be of order 100 %
    rel = {k: (on_grads[k] - ref).norm().item() / max(ref.norm().item(), 1e-12) for k, ref in off_grads.items()}
    print("\nrelative L2 of the conv weight gradients, kernel on / off:", rel)
    assert all(v <= 5e-2 for v in rel.values()), rel


def test_captured_step_runs_the_kernel_on_the_side_stream(gpu_device):
    """The bench's configuration: seld_graph.GraphedTrainStep puts the convolution weight gradients on a side stream
    (seld_overlap.launch_now, model_crnn._Conv3x3's job).  The kernel must run there for blocks 2-4 in the eager
    warm-up steps and in the captured one, and the replayed losses must track a run with the kernel switched off."""
    import model_crnn
    import seld_graph
    import seld_native
    import seld_overlap
    import trainer
    calls = []
    real = seld_native.conv3x3_wgrad

    def counted(x, dy, dw):
        calls.append((x.shape[1], torch.cuda.current_stream(x.device) == seld_overlap.side_stream(x.device, 1)))
        return real(x, dy, dw)

    g = torch.Generator().manual_seed(5)
    batches = [((torch.randn(4, 250, 4, 64, generator=g) * 20 - 30).to(gpu_device),
                ((torch.rand(4, 250, 648, generator=g) < 0.02).to(torch.int32) << 3).to(torch.uint16).to(gpu_device))
               for _ in range(6)]

    def run(fused):
        was = model_crnn._Conv3x3.fused_wgrad
        try:
            torch.manual_seed(0)
            model = trainer.prepare_model_for_device(model_crnn.SELD_CRNN(), gpu_device).train()
            for m in model.modules():
                if isinstance(m, torch.nn.Dropout):
                    m.p = 0.0
            model.rnn.dropout = 0.0
            model_crnn._Conv3x3.fused_wgrad = fused
            seld_native.conv3x3_wgrad = counted
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
            seld_native.conv3x3_wgrad = real
            model_crnn._Conv3x3.fused_wgrad = was

    on, on_err = run(True)
    assert on_err is None, on_err
    assert len(calls) >= 12 and len(calls) % 3 == 0, calls             # 3 eager steps + the capture, 3 blocks each
    assert sorted({c for c, _ in calls}) == [64, 128, 256] and all(side for _, side in calls), calls
    n_on = len(calls)
    off, _ = run(False)
    assert len(calls) == n_on
    rel = ((on - off).abs() / off.abs()).max().item()
    assert rel <= 5e-3, (on, off)
