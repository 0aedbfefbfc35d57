"""GPU tests of the guarded optimiser update (csrc/guard.hip, the guarded instantiation of csrc/adam.hip,
trainer.MasterWeightAdam): the deterministic global gradient norm, clipping, the non-finite step
skip and the weight EMA, against the float64 statement of tests/guard_ref.py and against the framework-op fallback of the
same optimiser -- stand-alone, inside a captured training step and under a two-rank data-parallel run."""
import json
import math
import os
import subprocess
import sys
from pathlib import Path

import pytest
import torch

import guard_ref

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent

# the tensor set of test_own_adam_kernel_matches_the_framework_path (ragged, 1-element and channels-last shapes, bf16 and
# fp32 alternating) extended to 111 tensors: three launches of 48; the 7-cycle gives every shape in both dtypes
SHAPES = [(9072, 512), (768, 256), (37,), (5, 3, 3, 3), (64, 4, 3, 3), (1,)] + \
    [(37,), (5, 3, 3, 3), (64, 4, 3, 3), (1,), (130, 33), (4099,), (3,)] * 15
LR0, LR1, WD = 1e-2, 2.5e-3, 1e-4


def _build(device, own=True, clip=0.0, skip=False, decay=0.0, guarded=True):
    import trainer
    g = torch.Generator().manual_seed(5)
    low, masters, others = [], [], []
    for i, shape in enumerate(SHAPES):
        t = torch.randn(*shape, generator=g).to(device)
        if len(shape) == 4:
            t = t.contiguous(memory_format=torch.channels_last)
        if i % 2 == 0:
            low.append(torch.nn.Parameter(t.to(torch.bfloat16)))
            masters.append(t.clone())
        else:
            others.append(torch.nn.Parameter(t.clone()))
    opt = trainer.MasterWeightAdam(low, masters, others, lr=torch.tensor(LR0, device=device), weight_decay=WD, fused=True,
                                   capturable=True)
    opt.own_kernel = own
    if guarded:
        opt.configure_guard(clip, skip, decay)
    return opt


def _draw(gen, scale=0.1):
    """Host gradients in the order low + others of _build."""
    order = [s for i, s in enumerate(SHAPES) if i % 2 == 0] + [s for i, s in enumerate(SHAPES) if i % 2 == 1]
    return [torch.randn(*s, generator=gen) * scale for s in order]


def _place(opt, grads, device):
    """p.grad <- the gradient in the parameter's dtype and layout; returns the stored tensors."""
    stored = []
    for p, gr in zip(opt._low + opt._others, grads):
        gr = gr.to(device).to(p.dtype)
        if p.dim() == 4:
            gr = gr.contiguous(memory_format=torch.channels_last)
        p.grad = gr
        stored.append(gr)
    return stored


def _state(opt):
    params = opt._masters + [p.data for p in opt._others]
    keys = opt._masters + opt._others
    out = {"param": params, "low": [p.data for p in opt._low],
           "exp_avg": [opt.state[k]["exp_avg"] for k in keys if opt.state[k]],
           "exp_avg_sq": [opt.state[k]["exp_avg_sq"] for k in keys if opt.state[k]],
           "step": [opt.state[k]["step"] for k in keys if opt.state[k]]}
    if opt.ema_tensors() is not None:
        out["ema"] = opt.ema_tensors()
    return out


def _snapshot(opt):
    return {k: [t.detach().clone() for t in v] for k, v in _state(opt).items()}


def _assert_equal(a, b, what=""):
    assert a.keys() == b.keys(), (what, a.keys(), b.keys())
    for k in a:
        assert len(a[k]) == len(b[k]), (what, k)
        for i, (x, y) in enumerate(zip(a[k], b[k])):
            assert torch.equal(x, y), (what, k, i)


def _f64_norm(stored, scale=1.0):
    return math.sqrt(sum(float((t.double() * scale).pow(2).sum().item()) for t in stored))


def test_gradient_norm_and_coefficient(gpu_device):
    """Within 2e-6 relative of the float64 norm of the SAME stored gradients: the fp32 chain ahead of the double stage is
    25 additions of non-negative terms (<= 32 * 2^-24 on the sum, half that on the root) plus one rounding of the result."""
    import seld_native
    opt = _build(gpu_device, guarded=False)
    partial = torch.zeros(seld_native.grad_norm_scratch_floats([math.prod(s) for s in SHAPES]), device=gpu_device)
    for scale_of_data in (1e-6, 0.1, 50.0):
        stored = _place(opt, _draw(torch.Generator().manual_seed(11), scale_of_data), gpu_device)
        assert len(stored) > 96
        guard = seld_native.new_guard_record(gpu_device)
        assert seld_native.multi_grad_norm(stored, guard, partial)
        first = guard.clone()
        rec = seld_native.read_guard(guard)
        want = _f64_norm(stored)
        rel = abs(rec["grad_norm"] - want) / want
        print(f"norm {rec['grad_norm']!r} vs float64 {want!r}: relative error {rel:.3e}")
        assert rel <= 2e-6
        assert rec["clip_coef"] == 1.0 and rec["apply"] and rec["steps_skipped"] == 0 and rec["steps_clipped"] == 0
        assert seld_native.multi_grad_norm(stored, guard, partial)                   # bit-identical on a second call
        assert torch.equal(guard[:4].view(torch.int32), first[:4].view(torch.int32))
        # grad_scale
        assert seld_native.multi_grad_norm(stored, guard, partial, grad_scale=0.5)
        half = seld_native.read_guard(guard)["grad_norm"]
        want_half = _f64_norm(stored, 0.5)
        assert abs(half - want_half) / want_half <= 2e-6
        # coefficient: the fp32 evaluation of torch's formula on the kernel's own norm, exactly
        max_norm = float(torch.tensor(0.5 * want, dtype=torch.float32))
        assert seld_native.multi_grad_norm(stored, guard, partial, max_norm=max_norm)
        rec = seld_native.read_guard(guard)
        norm32 = torch.tensor(rec["grad_norm"], dtype=torch.float32)
        coef32 = torch.clamp(torch.tensor(max_norm, dtype=torch.float32) / (norm32 + torch.tensor(1e-6, dtype=torch.float32)),
                             max=1.0)
        assert rec["clip_coef"] == float(coef32)
        want_coef = min(1.0, max_norm / (want + 1e-6))
        print(f"coef {rec['clip_coef']!r} vs float64 {want_coef!r}")
        assert abs(rec["clip_coef"] - want_coef) / want_coef <= 4e-6
        assert rec["steps_clipped"] == 1 and rec["steps_skipped"] == 0
        assert seld_native.multi_grad_norm(stored, guard, partial, max_norm=0.0)
        assert seld_native.read_guard(guard)["clip_coef"] == 1.0
    # a layout the kernel cannot walk is refused, nothing written
    guard = seld_native.new_guard_record(gpu_device)
    assert not seld_native.multi_grad_norm([torch.zeros(8, 8, device=gpu_device).t()[:, :3]], guard, partial)
    assert guard.abs().sum().item() == 0


def test_inactive_guard_is_bit_identical_to_the_plain_update(gpu_device):
    a = _build(gpu_device, clip=1e9, skip=True)
    b = _build(gpu_device, guarded=False)
    gen = torch.Generator().manual_seed(9)
    for step in range(1, 9):
        if step == 5:
            for opt in (a, b):
                opt.param_groups[0]["lr"].fill_(LR1)
        grads = _draw(gen)
        for opt in (a, b):
            _place(opt, grads, gpu_device)
            opt.step()
    assert a.own_steps == 8 and b.own_steps == 8 and a.guard_active and not b.guard_active
    _assert_equal(_state(a), _state(b))
    assert all(float(s) == 8.0 for s in _state(a)["step"])
    report = a.guard_report()
    assert report["steps_skipped"] == 0 and report["steps_clipped"] == 0 and report["clip_coef"] == 1.0


def test_active_clipping_matches_the_reference_and_the_fallback(gpu_device):
    """max_norm = half the first step's measured norm (read from the guard), so every step clips.  Tolerance: the plain
    update's 2e-6 * max|param| plus steps * lr * 4 * 2e-6 -- the norm's tolerance carried through at most `steps` updates,
    each bounded by a few lr."""
    import seld_native
    gen = torch.Generator().manual_seed(9)
    all_grads = [_draw(gen) for _ in range(8)]
    probe = _build(gpu_device, clip=1.0)
    stored = _place(probe, all_grads[0], gpu_device)
    assert seld_native.multi_grad_norm(stored, probe._guard, probe._partial)
    max_norm = 0.5 * probe.guard_report()["grad_norm"]
    a = _build(gpu_device, clip=max_norm)
    b = _build(gpu_device, own=False, clip=max_norm)
    ref = guard_ref.GuardedAdamRef(a._masters + [p.data for p in a._others], lr=LR0, weight_decay=WD, max_norm=max_norm)
    for step in range(1, 9):
        if step == 5:
            ref.lr = LR1
            for opt in (a, b):
                opt.param_groups[0]["lr"].fill_(LR1)
        stored = [t.clone() for t in _place(a, all_grads[step - 1], gpu_device)]   # (the fallback scales its fp32 gradients in place)
        _place(b, all_grads[step - 1], gpu_device)
        for opt in (a, b):
            opt.step()
        assert ref.step(stored) and ref.coef < 1.0
    assert a.own_steps == 8 and b.own_steps == 0
    assert a.guard_report()["steps_clipped"] == 8 and b.guard_report()["steps_clipped"] == 8
    assert a.guard_report()["steps_skipped"] == 0
    assert abs(a.guard_report()["clip_coef"] - ref.coef) <= 4e-6 * ref.coef
    extra = 8 * LR0 * 4 * 2e-6
    worst = 0.0
    for i, (x, y, r) in enumerate(zip(_state(a)["param"], _state(b)["param"], ref.p)):
        tol = 2e-6 * (r.abs().max().item() + 1e-6) + extra
        err_ref, err_fb = (x.double().cpu() - r).abs().max().item(), (x - y).abs().max().item()
        worst = max(worst, err_ref / tol, err_fb / tol)
        assert err_ref <= tol, (i, err_ref, tol)
        assert err_fb <= tol, (i, err_fb, tol)
    print(f"worst error / tolerance = {worst:.3f}")
    for pa, m in zip(a._low, a._masters):
        assert torch.equal(pa.data, m.to(torch.bfloat16))
    assert all(float(s) == 8.0 for s in _state(a)["step"] + _state(b)["step"])


# (position in low + others, what): the last element of a ragged bf16 tensor (37 elements: the tail path) and the last
# element of an fp32 one (135 elements, channels-last)
_N_LOW = len([i for i in range(len(SHAPES)) if i % 2 == 0])
_TARGETS = {"bf16": 1, "fp32": _N_LOW + 1}


@pytest.mark.parametrize("value", [float("inf"), float("nan")])
@pytest.mark.parametrize("target", ["bf16", "fp32"])
def test_non_finite_step_is_skipped(gpu_device, target, value):
    """A numeric inf / NaN planted in ONE gradient element: with the skip armed nothing changes in that step and the run
    continues exactly as if the step had never happened; without it the masters end non-finite."""
    gen = torch.Generator().manual_seed(21)
    good = [_draw(gen) for _ in range(4)]
    bad = [t.clone() for t in _draw(gen)]

    def run(opt, with_bad):
        before = after = None
        for k in range(4):
            if with_bad and k == 2:
                stored = _place(opt, bad, gpu_device)
                t = stored[_TARGETS[target]]
                assert t.dtype == (torch.bfloat16 if target == "bf16" else torch.float32)
                t.as_strided((t.numel(),), (1,))[-1] = value
                before = _snapshot(opt)
                opt.step()
                after = _snapshot(opt)
            _place(opt, good[k], gpu_device)
            opt.step()
        return before, after

    assert SHAPES[2 * _TARGETS["bf16"]] == (37,) and SHAPES[2 * (_TARGETS["fp32"] - _N_LOW) + 1] == (5, 3, 3, 3)
    a = _build(gpu_device, clip=1e9, skip=True, decay=0.99)
    before, after = run(a, True)
    _assert_equal(before, after, "skipped step")
    assert "ema" in before and all(float(s) == 2.0 for s in before["step"])
    report = a.guard_report()
    assert report["steps_skipped"] == 1 and a.own_steps == 5
    twin = _build(gpu_device, clip=1e9, skip=True, decay=0.99)
    run(twin, False)
    _assert_equal(_state(a), _state(twin), "after the skipped step")
    assert all(float(s) == 4.0 for s in _state(a)["step"]) and twin.guard_report()["steps_skipped"] == 0
    # the framework-op fallback skips the same way (found_inf of torch's fused Adam)
    fb = _build(gpu_device, own=False, clip=1e9, skip=True, decay=0.99)
    before, after = run(fb, True)
    _assert_equal(before, after, "skipped step, fallback")
    assert fb.guard_report()["steps_skipped"] == 1 and all(float(s) == 4.0 for s in _state(fb)["step"])
    # without the skip the same sequence poisons the weights: the test would catch a guard that does nothing
    loose = _build(gpu_device, clip=1e9, skip=False, decay=0.99)
    run(loose, True)
    assert not all(bool(torch.isfinite(p).all()) for p in _state(loose)["param"])
    assert loose.guard_report()["steps_skipped"] == 0


def test_weight_ema(gpu_device):
    a = _build(gpu_device, decay=0.99)
    b = _build(gpu_device, own=False, decay=0.99)
    plain = _build(gpu_device, guarded=False)
    assert plain.ema_tensors() is None and _build(gpu_device, clip=1.0).ema_tensors() is None
    assert a._guard is None                                     # EMA alone needs no norm pass and no record
    ref = guard_ref.GuardedAdamRef(a._masters + [p.data for p in a._others], lr=LR0, weight_decay=WD, ema_decay=0.99)
    for e, p in zip(a.ema_tensors(), _state(a)["param"]):
        assert torch.equal(e, p) and e.data_ptr() != p.data_ptr()
    gen = torch.Generator().manual_seed(9)
    for step in range(1, 9):
        if step == 5:
            ref.lr = LR1
            for opt in (a, b, plain):
                opt.param_groups[0]["lr"].fill_(LR1)
        grads = _draw(gen)
        for opt in (a, b, plain):
            stored = _place(opt, grads, gpu_device)
            opt.step()
        ref.step(stored)
    assert a.own_steps == 8 and b.own_steps == 0
    _assert_equal({k: v for k, v in _state(a).items() if k != "ema"}, _state(plain), "EMA must not change the update")
    for i, (x, y, r, p) in enumerate(zip(a.ema_tensors(), b.ema_tensors(), ref.ema, ref.p)):
        tol = 2e-6 * (p.abs().max().item() + 1e-6)
        assert (x.double().cpu() - r).abs().max().item() <= tol, i
        assert (x - y).abs().max().item() <= tol, i
    assert max((e - p).abs().max().item() for e, p in zip(a.ema_tensors(), _state(a)["param"])) > 1e-3
    assert set(a.state_dict()) == {"state", "param_groups"}
    assert all(set(v) == {"step", "exp_avg", "exp_avg_sq"} for v in a.state_dict()["state"].values())


# ---------------------------------------------------------------------------------------------- captured step

class _ScaledLoss:
    """The criterion with its total multiplied by a static device scalar (1.0; inf for one iteration): the forward pass
    and BatchNorm's statistics stay finite, every gradient of that iteration does not."""

    def __init__(self, inner, device):
        self.inner = inner
        self.scalar = torch.ones((), device=device)

    def loss_tensor(self, predictions, labels):
        total, term = self.inner.loss_tensor(predictions, labels)
        return total * self.scalar, term


def _captured(device, graphs, batches, poison_at=None, clip=1e-3):
    import seld_graph
    import trainer
    cfg = trainer.config
    keys = ("MODEL_TYPE", "CRNN_CNN_CHANNELS", "GRAD_CLIP_NORM", "SKIP_NONFINITE_STEPS", "EMA_DECAY")
    saved = {k: getattr(cfg, k) for k in keys}
    cfg.MODEL_TYPE, cfg.CRNN_CNN_CHANNELS = "crnn", [16, 16, 32, 32]
    cfg.GRAD_CLIP_NORM, cfg.SKIP_NONFINITE_STEPS, cfg.EMA_DECAY = clip, True, 0.99
    try:
        torch.manual_seed(0)
        model = trainer.prepare_model_for_device(trainer.build_model((18, 36)), device).train()
        for m in model.modules():
            if isinstance(m, torch.nn.Dropout):
                m.p = 0.0
            if isinstance(m, torch.nn.GRU):
                m.dropout = 0.0
        trainer.enable_master_weights(model, device)
        crit = _ScaledLoss(trainer.SMRSELDLoss("mse", 1.0, grid_size=(18, 36)), device)
        opt = trainer.make_optimizer(model, 1e-3, device, capturable=True)
        assert opt.guard_active and opt.ema_tensors() is not None
        step = seld_graph.GraphedTrainStep(model, crit, opt, device, autocast=lambda: trainer.autocast_context(device),
                                           use_graphs=graphs)
        losses, around = [], None
        for i, (x, m) in enumerate(batches):
            if i == poison_at:
                crit.scalar.fill_(float("inf"))
                before = _snapshot(opt)
            total, _ = step(x, m)
            losses.append(total.clone())
            if i == poison_at:
                around = (before, _snapshot(opt))
                crit.scalar.fill_(1.0)
        losses = torch.stack(losses).cpu()
        stats = step.stats()
        step.close()
        report = opt.guard_report()
        sd = {k: v.detach().float().cpu().clone() for k, v in trainer.model_state_dict(model).items()}
        ema = {k: v.detach().float().cpu().clone() for k, v in trainer.ema_state_dict(model, opt).items()}
        trainer.disable_master_weights(model)
        return {"losses": losses, "sd": sd, "ema": ema, "stats": stats, "report": report, "around": around,
                "own_steps": opt.own_steps}
    finally:
        for k, v in saved.items():
            setattr(cfg, k, v)


def _batches(device, n, batch=8, seed=3):
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(n):
        x = (torch.randn(batch, 250, 4, 64, generator=g) * 20 - 30).to(device)
        m = ((torch.rand(batch, 250, 648, generator=g) < 0.02).to(torch.int32) << 3).to(torch.uint16).to(device)
        out.append((x, m))
    return out


def test_captured_step_with_clipping_and_ema(gpu_device):
    batches = _batches(gpu_device, 16)
    was = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    try:
        eager = _captured(gpu_device, False, batches)
        again = _captured(gpu_device, False, batches)
        graph = _captured(gpu_device, True, batches)
        poisoned = _captured(gpu_device, True, batches, poison_at=9)
    finally:
        torch.backends.cudnn.deterministic = was
    assert graph["stats"]["capture_error"] is None and graph["stats"]["graphs"] == 1 and graph["stats"]["replays"] == 13
    assert eager["stats"]["graphs"] == 0
    assert eager["own_steps"] == 16 and graph["own_steps"] == 4          # (host-side count: 3 warm-ups + the capture)
    for run in (eager, graph):
        assert run["report"]["steps_clipped"] == 16 and run["report"]["steps_skipped"] == 0
        assert run["report"]["clip_coef"] < 1.0
    assert torch.isfinite(eager["losses"]).all() and eager["losses"][-1] < eager["losses"][0]
    assert torch.equal(eager["losses"], again["losses"]), "the eager loop must be reproducible for this comparison"
    assert torch.equal(eager["losses"], graph["losses"]), (eager["losses"] - graph["losses"]).abs().max().item()
    for k in eager["sd"]:
        assert torch.equal(eager["sd"][k], graph["sd"][k]), k
        assert torch.equal(eager["ema"][k], graph["ema"][k]), k
    assert any(not torch.equal(eager["sd"][k], eager["ema"][k]) for k in eager["sd"])
    # one replay with a non-finite backward pass: skipped, weights / state / EMA untouched, training goes on
    assert poisoned["stats"]["capture_error"] is None and poisoned["stats"]["replays"] == 13
    before, after = poisoned["around"]
    _assert_equal(before, after, "skipped replay")
    assert poisoned["report"]["steps_skipped"] == 1 and poisoned["report"]["steps_clipped"] == 15
    losses = poisoned["losses"]
    assert not torch.isfinite(losses[9]) and torch.isfinite(losses[:9]).all() and torch.isfinite(losses[10:]).all()
    assert torch.equal(losses[:9], graph["losses"][:9])
    print('losses around the skipped replay:', losses.tolist())
    assert losses[10:].mean() < losses[:9].mean() and losses[-1] < losses[0]          # training goes on
    assert all(torch.isfinite(v).all() for v in poisoned["sd"].values())
    assert all(torch.isfinite(v).all() for v in poisoned["ema"].values())


# ---------------------------------------------------------------------------------------------- data parallel

def test_data_parallel_replicas_share_the_guard_decision(gpu_device):
    """ONE two-rank launch (gloo, both ranks on GPU 0) of tests/ddp_guard_worker.py with clipping active: every rank holds
    bit-identical reduced gradients and the norm is a fixed-order sum, so norm, coefficient, weights and EMA are bit-equal
    across ranks without a collective for the guard -- with the overlapped exchange and with the blocking one alike."""
    env = dict(os.environ, SELD_DIST_BACKEND="gloo", MASTER_ADDR="127.0.0.1")
    port = 30700 + os.getpid() % 90
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), str(ROOT / "tests" / "ddp_guard_worker.py"), "1e-3"]
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600, cwd=str(ROOT))
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [json.loads(l.split("RANKLINE ", 1)[1]) for l in out.stdout.splitlines() if "RANKLINE " in l]
    runs = {(d["mode"], d["rank"]): d for d in lines}
    assert set(runs) == {("staged", 0), ("staged", 1), ("blocking", 0), ("blocking", 1)}
    for mode in ("staged", "blocking"):
        a, b = runs[(mode, 0)], runs[(mode, 1)]
        for d in (a, b):
            assert d["capture_error"] is None and d["replays"] == 7 and d["own_steps"] == 4
            assert d["report"]["steps_clipped"] == 10 and d["report"]["steps_skipped"] == 0
            assert 0.0 < d["report"]["clip_coef"] < 1.0 and all(math.isfinite(v) for v in d["losses"])
        assert a["norm_coef_bits"] == b["norm_coef_bits"], mode
        assert a["digest"] == b["digest"] and a["ema_digest"] == b["ema_digest"], mode
        assert a["losses"] != b["losses"]                                   # per-rank batches
    assert runs[("staged", 0)]["digest"] == runs[("blocking", 0)]["digest"]
    assert runs[("staged", 0)]["ema_digest"] == runs[("blocking", 0)]["ema_digest"]
    assert runs[("staged", 0)]["norm_coef_bits"] == runs[("blocking", 0)]["norm_coef_bits"]
