"""CPU tests of the guarded optimiser update (gradient-norm clipping, non-finite step skip, weight EMA; DESIGN.md section
12): the C ABI and its binding, the config surface, the float64 reference against the framework, the checkpoint format and
the compiler's resource report of the new kernels.  No GPU compute here."""
import re
import subprocess
from pathlib import Path

import pytest
import torch

import guard_ref

ROOT = Path(__file__).resolve().parent.parent
PKG = ROOT / "sound-event-localization-detection_amd"
HEADER = ROOT / "include" / "seld_hip.h"

ARITY = {"seld_multi_grad_norm_scratch": 3, "seld_multi_grad_norm": 11, "seld_multi_adam_guarded": 19}


def test_header_declares_and_library_exports_the_guard_entry_points():
    import seld_native
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    lib = seld_native.load_library()
    for name, arity in ARITY.items():
        m = re.search(r"\b" + name + r"\s*\(([^)]*)\)", text)
        assert m, f"{name} is not declared in include/seld_hip.h"
        assert len(m.group(1).split(",")) == arity, name
        fn = getattr(lib, name)
        assert fn.argtypes is not None and len(fn.argtypes) == arity, name
    # the guard record's layout is fixed in the header: 8 words
    body = re.search(r"typedef struct seld_guard_record \{(.*?)\} seld_guard_record;", text, flags=re.S).group(1)
    fields = re.findall(r"\b(float|int32_t)\s+(\w+)(\[(\d+)\])?;", body)
    assert [f[1] for f in fields] == ["grad_norm", "clip_coef", "apply", "skipped", "steps_skipped", "steps_clipped",
                                      "reserved"]
    assert sum(int(f[3] or 1) for f in fields) == seld_native.GUARD_WORDS == 8
    assert seld_native.grad_norm_scratch_floats([1, 4096, 4097, 3 * 4096]) == 1 + 1 + 2 + 3
    assert callable(seld_native.multi_grad_norm) and callable(seld_native.multi_adam_guarded)


def test_config_switches_default_to_off():
    from config import Config
    assert Config.GRAD_CLIP_NORM == 0.0 and Config.SKIP_NONFINITE_STEPS is False
    assert Config.EMA_DECAY == 0.0 and Config.EVAL_USE_EMA is False


class _Tiny(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.conv = torch.nn.Conv2d(2, 4, 3)
        self.bn = torch.nn.BatchNorm2d(4)
        self.fc = torch.nn.Linear(4, 3)


def _with_config(**values):
    import trainer
    saved = {k: getattr(trainer.config, k) for k in values}
    for k, v in values.items():
        setattr(trainer.config, k, v)
    return saved


def _restore(saved):
    import trainer
    for k, v in saved.items():
        setattr(trainer.config, k, v)


@pytest.mark.parametrize("switch", [{"GRAD_CLIP_NORM": 1.0}, {"SKIP_NONFINITE_STEPS": True}, {"EMA_DECAY": 0.99}])
def test_make_optimizer_refuses_a_guard_without_the_master_weight_path(switch):
    import trainer
    model = _Tiny()
    opt = trainer.make_optimizer(model, 1e-3, torch.device("cpu"))               # all off: as before
    assert type(opt) is torch.optim.Adam and opt.param_groups[0]["weight_decay"] == trainer.config.WEIGHT_DECAY
    saved = _with_config(**switch)
    try:
        with pytest.raises(ValueError, match="master-weight"):
            trainer.make_optimizer(model, 1e-3, torch.device("cpu"))
    finally:
        _restore(saved)


def test_out_of_range_switches_are_refused():
    import trainer
    for bad in ({"GRAD_CLIP_NORM": -1.0}, {"GRAD_CLIP_NORM": float("inf")}, {"EMA_DECAY": 1.0}, {"EMA_DECAY": -0.1}):
        saved = _with_config(**bad)
        try:
            with pytest.raises(ValueError):
                trainer.make_optimizer(_Tiny(), 1e-3, torch.device("cpu"))
        finally:
            _restore(saved)


@pytest.mark.parametrize("max_norm,decay", [(0.0, 0.0), (0.3, 0.99), (1e9, 0.9)])
def test_guard_ref_agrees_with_the_framework(max_norm, decay):
    """clip_grad_norm_ -> torch.optim.Adam(weight_decay) -> _foreach_lerp_ on float64 CPU tensors against guard_ref:
    1e-12 relative over 8 steps (the GPU tests are graded against guard_ref)."""
    g = torch.Generator().manual_seed(4)
    shapes = [(33, 7), (5,), (1,), (4, 3, 3, 3)]
    params = [torch.nn.Parameter(torch.randn(*s, generator=g, dtype=torch.float64)) for s in shapes]
    ema = [p.detach().clone() for p in params]
    opt = torch.optim.Adam(params, lr=1e-2, weight_decay=1e-4)
    ref = guard_ref.GuardedAdamRef([p.data for p in params], lr=1e-2, weight_decay=1e-4, max_norm=max_norm, ema_decay=decay)
    for step in range(8):
        if step == 4:
            opt.param_groups[0]["lr"] = ref.lr = 2.5e-3
        grads = [torch.randn(*s, generator=g, dtype=torch.float64) * 0.1 for s in shapes]
        for p, gr in zip(params, grads):
            p.grad = gr.clone()
        if max_norm > 0:
            total = torch.nn.utils.clip_grad_norm_(params, max_norm)
        else:
            total = torch.linalg.vector_norm(torch.cat([gr.flatten() for gr in grads]))
        opt.step()
        if decay > 0:
            torch._foreach_lerp_(ema, [p.data for p in params], 1.0 - decay)
        assert ref.step(grads)
        assert abs(ref.norm - float(total)) <= 1e-12 * float(total)
    assert ref.clipped == (8 if max_norm == 0.3 else 0) and ref.skipped == 0 and ref.step_count == 8
    for p, r in zip(params, ref.p):
        assert (p.data - r).abs().max().item() <= 1e-12 * r.abs().max().item()
    if decay > 0:
        for e, r in zip(ema, ref.ema):
            assert (e - r).abs().max().item() <= 1e-12 * r.abs().max().item()
    else:
        assert ref.ema is None


def test_guard_ref_skips_a_non_finite_step():
    p = [torch.ones(5, dtype=torch.float64)]
    ref = guard_ref.GuardedAdamRef(p, lr=1e-2, skip_nonfinite=True, ema_decay=0.9, max_norm=1.0)
    assert ref.step([torch.full((5,), 0.5, dtype=torch.float64)])
    before = (ref.p[0].clone(), ref.m[0].clone(), ref.v[0].clone(), ref.ema[0].clone(), ref.step_count)
    bad = torch.full((5,), 0.5, dtype=torch.float64)
    bad[4] = float("nan")
    assert not ref.step([bad])
    assert torch.equal(ref.p[0], before[0]) and torch.equal(ref.m[0], before[1]) and torch.equal(ref.v[0], before[2])
    assert torch.equal(ref.ema[0], before[3]) and ref.step_count == before[4] and ref.skipped == 1
    loose = guard_ref.GuardedAdamRef(p, lr=1e-2, skip_nonfinite=False)
    assert loose.step([bad]) and not torch.isfinite(loose.p[0]).all()


def _cpu_master_setup(decay):
    """A CPU model in the master-weight arrangement (what enable_master_weights builds on a ROCm device) and its
    MasterWeightAdam, with EMA alone: no device record is needed for that."""
    import trainer
    torch.manual_seed(0)
    model = _Tiny()
    low, masters, names = [], [], {}
    for mod_name, module in model.named_modules():
        if isinstance(module, (torch.nn.Conv2d, torch.nn.Linear)):
            p = module.weight
            masters.append(p.detach().clone())
            p.data = p.data.to(torch.bfloat16)
            low.append(p)
            names[f"{mod_name}.weight"] = masters[-1]
    model._seld_master_weights = (low, masters, names)
    low_ids = {id(p) for p in low}
    others = [p for p in model.parameters() if id(p) not in low_ids]
    opt = trainer.MasterWeightAdam(low, masters, others, lr=1e-3)
    if decay:
        opt.configure_guard(0.0, False, decay)
    return model, opt


def test_checkpoint_payload_keys_and_ema_state_dict():
    import trainer
    model, opt = _cpu_master_setup(0.0)
    assert opt.ema_tensors() is None and not opt.guard_active
    payload = trainer.checkpoint_payload(3, model, opt, 0.5, 0.6)
    assert set(payload) == {"epoch", "model_state_dict", "optimizer_state_dict", "train_loss", "test_loss", "config"}
    assert trainer.ema_state_dict(model, opt) is None

    model, opt = _cpu_master_setup(0.99)
    saved = _with_config(EMA_DECAY=0.99)
    try:
        for e in opt.ema_tensors():
            e.add_(1.0)                                     # tell the EMA apart from the live weights
        payload = trainer.checkpoint_payload(3, model, opt, 0.5, 0.6)
    finally:
        _restore(saved)
    assert set(payload) == {"epoch", "model_state_dict", "optimizer_state_dict", "train_loss", "test_loss", "config",
                            "ema_state_dict"}
    ema, live = payload["ema_state_dict"], payload["model_state_dict"]
    assert list(ema.keys()) == list(live.keys()) == list(_Tiny().state_dict().keys())
    param_names = {n for n, _ in model.named_parameters()}
    for k in ema:
        assert ema[k].dtype == live[k].dtype and (not ema[k].is_floating_point() or ema[k].dtype == torch.float32), k
        if k in param_names:
            assert torch.equal(ema[k], live[k] + 1.0), k
        else:
            assert torch.equal(ema[k], live[k]), k          # buffers: the live model's
    assert set(opt.state_dict()) == {"state", "param_groups"}          # EMA lives outside the optimiser state
    fresh = _Tiny()
    fresh.load_state_dict(ema)


def test_use_ema_selection():
    import trainer
    with_ema = {"model_state_dict": {"w": 1}, "ema_state_dict": {"w": 2}}
    without = {"model_state_dict": {"w": 1}}
    assert trainer.select_state_dict(with_ema) == {"w": 1}                 # EVAL_USE_EMA is off by default
    assert trainer.select_state_dict(with_ema, use_ema=True) == {"w": 2}
    assert trainer.select_state_dict(without, use_ema=False) == {"w": 1}
    with pytest.raises(KeyError, match="ema_state_dict"):
        trainer.select_state_dict(without, use_ema=True)
    saved = _with_config(EVAL_USE_EMA=True)
    try:
        assert trainer.select_state_dict(with_ema) == {"w": 2}
        assert trainer.select_state_dict(with_ema, use_ema=False) == {"w": 1}
        with pytest.raises(KeyError):
            trainer.select_state_dict(without)
    finally:
        _restore(saved)


def test_guard_kernels_do_not_spill():
    """The compiler's resource report (-Rpass-analysis=kernel-resource-usage): 0 scratch bytes per lane for the two norm
    kernels and for both instantiations of the Adam kernel."""
    csrc = PKG / "csrc"
    wanted = {"guard.hip": ("grad_sumsq_kernel", "guard_finish_kernel"),
              "adam.hip": ("multi_adam_kernel", "multi_adam_guarded_kernel")}
    for name, kernels in wanted.items():
        run = subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", f"-I{ROOT / 'include'}",
                              "-Rpass-analysis=kernel-resource-usage", "-c", str(csrc / name), "-o", "/dev/null"],
                             capture_output=True, text=True)
        assert run.returncode == 0, run.stderr[-2000:]
        found, current = {}, None
        for line in run.stderr.splitlines():
            m = re.search(r"Function Name: (\S+)", line)
            if m:
                current = m.group(1)
            m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
            if m and current:
                found[current] = int(m.group(1))
        for kernel in kernels:
            hits = {k: v for k, v in found.items() if re.search(r"\d" + kernel + "E", k)}
            assert hits, (name, kernel, sorted(found))
            assert all(v == 0 for v in hits.values()), (name, hits)
