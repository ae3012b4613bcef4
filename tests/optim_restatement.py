"""The AdamW update and the gradient clip as plain float64 torch expressions: the truth of tests/test_gpu_optim.py and
tools/optim_parity.py.  tests/test_optim_cpu.py pins it to torch.optim.AdamW on float64 tensors, so it restates the real
optimizer and not the code under test."""
import math

import torch


def adamw_update(p, g, m, v, step, lr, betas, eps, weight_decay):
    """One step of torch.optim.AdamW (decoupled weight decay, no amsgrad) on float64 tensors -> (p, m, v), new tensors.
    step: this step's number, >= 1."""
    beta1, beta2 = betas
    p, g, m, v = p.double(), g.double(), m.double(), v.double()
    p = p * (1 - lr * weight_decay)
    m = m + (g - m) * (1 - beta1)
    v = v * beta2 + (1 - beta2) * g * g
    step_size = lr / (1 - beta1 ** step)
    bc2_sqrt = math.sqrt(1 - beta2 ** step)
    p = p - step_size * m / (v.sqrt() / bc2_sqrt + eps)
    return p, m, v


class Adamw64:
    """Float64 state of a list of tensors: step(i, grad, **hyper) updates entry i; entries count their own steps."""

    def __init__(self, params):
        self.p = [t.detach().double().cpu().clone() for t in params]
        self.m = [torch.zeros_like(t) for t in self.p]
        self.v = [torch.zeros_like(t) for t in self.p]
        self.steps = [0] * len(self.p)

    def step(self, i, grad, lr, betas, eps, weight_decay):
        self.steps[i] += 1
        self.p[i], self.m[i], self.v[i] = adamw_update(self.p[i], grad.detach().double().cpu(), self.m[i], self.v[i], self.steps[i], lr,
                                                       betas, eps, weight_decay)


def total_norm(grads):
    """The 2-norm of a list of gradients viewed as one vector, float64 -> Python float."""
    return math.sqrt(sum(float((g.detach().double() ** 2).sum()) for g in grads))


def clip_coef(norm, max_norm):
    """clip_grad_norm_'s coefficient min(max_norm / (norm + 1e-6), 1) in IEEE fp32 from the fp32 norm -> 0-dim fp32 CPU tensor."""
    norm = norm.detach().to("cpu", torch.float32)
    c = torch.tensor(float(max_norm), dtype=torch.float32) / (norm + torch.tensor(1e-6, dtype=torch.float32))
    return torch.clamp(c, max=1.0)
