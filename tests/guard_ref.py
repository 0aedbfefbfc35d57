"""Float64 statement of the guarded optimiser update, written from its definition:

    n    = sqrt(sum over ALL optimiser tensors of (g * grad_scale)^2)          g as stored (bf16 values are exact in fp64)
    coef = 1 if max_norm <= 0 else min(1, max_norm / (n + 1e-6))
    if skip_nonfinite and not isfinite(n):  nothing changes (p, m, v, step, ema);  skipped += 1
    else:  step += 1;  Adam with L2 weight decay on g * grad_scale * coef (weight decay added after clipping);
           ema += (1 - decay) * (p_new - ema);  clipped += (coef < 1)

The yardstick of tests/test_guard_gpu.py; tests/test_guard_cpu.py pins it against clip_grad_norm_ + torch.optim.Adam +
_foreach_lerp_ on float64 CPU tensors."""
import math

import torch


class GuardedAdamRef:
    def __init__(self, params, lr, weight_decay=0.0, betas=(0.9, 0.999), eps=1e-8, max_norm=0.0, skip_nonfinite=False,
                 ema_decay=0.0, grad_scale=1.0):
        self.p = [t.detach().double().cpu().clone() for t in params]
        self.m = [torch.zeros_like(t) for t in self.p]
        self.v = [torch.zeros_like(t) for t in self.p]
        self.ema = [t.clone() for t in self.p] if ema_decay > 0 else None
        self.lr, self.weight_decay, self.betas, self.eps = float(lr), float(weight_decay), betas, float(eps)
        self.max_norm, self.skip_nonfinite, self.ema_decay = float(max_norm), bool(skip_nonfinite), float(ema_decay)
        self.grad_scale = float(grad_scale)
        self.step_count = self.skipped = self.clipped = 0
        self.norm = self.coef = None

    def step(self, grads):
        g = [t.detach().double().cpu() * self.grad_scale for t in grads]
        n = math.sqrt(sum(float((t * t).sum()) for t in g))
        coef = 1.0 if self.max_norm <= 0 else min(1.0, self.max_norm / (n + 1e-6))
        self.norm, self.coef = n, coef
        if self.skip_nonfinite and not math.isfinite(n):
            self.skipped += 1
            return False
        self.step_count += 1
        b1, b2 = self.betas
        for i, gi in enumerate(g):
            gi = gi * coef + self.weight_decay * self.p[i]
            self.m[i] = b1 * self.m[i] + (1 - b1) * gi
            self.v[i] = b2 * self.v[i] + (1 - b2) * gi * gi
            denom = self.v[i].sqrt() / math.sqrt(1 - b2 ** self.step_count) + self.eps
            self.p[i] = self.p[i] - (self.lr / (1 - b1 ** self.step_count)) * self.m[i] / denom
            if self.ema is not None:
                self.ema[i] = self.ema[i] + (1 - self.ema_decay) * (self.p[i] - self.ema[i])
        self.clipped += int(coef < 1)
        return True
