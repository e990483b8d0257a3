"""The two ``optimizer_name`` values the reference takes from ``torch_optimizer`` (``sc/utils/parameter.py:34-39``,
``torch-optimizer==0.1.0``), restated as ``torch.optim.Optimizer`` subclasses: the oracle of the fused HIP updates
(``raae_optim_step``).  Not a conftest: tests import it.

Both follow the ``step()`` of torch_optimizer 0.1.0 line for line -- the same torch ops on the same fp32 tensors, the
per-step scalars as Python floats, an int ``state["step"]`` advanced once per step, the state keys ``step``,
``exp_avg`` and ``exp_avg_sq``, ``ValueError`` for ``lr <= 0`` at construction.
"""
import math

import torch


class RAdam(torch.optim.Optimizer):
    """torch_optimizer.RAdam (0.1.0): rectified Adam (Liu et al. 2019) with decoupled weight decay, including the
    class's 10-entry cache of ``(step, N_sma, step_size)`` keyed on ``step % 10``.  The original works on
    ``.float()`` copies of the gradient and the parameter: ``compute_dtype`` (a subclass may set float64 to pin a
    float64 reference to these very lines)."""

    compute_dtype = torch.float32

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0):
        if lr <= 0.0:
            raise ValueError(f"Invalid learning rate: {lr}")
        if eps < 0.0:
            raise ValueError(f"Invalid epsilon value: {eps}")
        if not 0.0 <= betas[0] < 1.0 or not 0.0 <= betas[1] < 1.0:
            raise ValueError(f"Invalid beta parameters: {betas}")
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay,
                        buffer=[[None, None, None] for _ in range(10)])
        super().__init__(params, defaults)

    @torch.no_grad()
    def step(self, closure=None):
        for group in self.param_groups:
            lr, weight_decay, eps = group["lr"], group["weight_decay"], group["eps"]
            beta1, beta2 = group["betas"]
            for p in group["params"]:
                if p.grad is None:
                    continue
                grad = p.grad.to(self.compute_dtype)
                p_fp32 = p.to(self.compute_dtype)
                state = self.state[p]
                if len(state) == 0:
                    state["step"] = 0
                    state["exp_avg"] = torch.zeros_like(p_fp32)
                    state["exp_avg_sq"] = torch.zeros_like(p_fp32)
                exp_avg, exp_avg_sq = state["exp_avg"], state["exp_avg_sq"]
                exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=1 - beta2)
                exp_avg.mul_(beta1).add_(grad, alpha=1 - beta1)
                state["step"] += 1
                buffered = group["buffer"][int(state["step"] % 10)]
                if state["step"] == buffered[0]:
                    n_sma, step_size = buffered[1], buffered[2]
                else:
                    buffered[0] = state["step"]
                    beta2_t = beta2 ** state["step"]
                    n_sma_max = 2 / (1 - beta2) - 1
                    n_sma = n_sma_max - 2 * state["step"] * beta2_t / (1 - beta2_t)
                    buffered[1] = n_sma
                    if n_sma >= 5:
                        step_size = (lr * math.sqrt((1 - beta2_t) * (n_sma - 4) / (n_sma_max - 4) * (n_sma - 2) / n_sma *
                                                    n_sma_max / (n_sma_max - 2)) / (1 - beta1 ** state["step"]))
                    else:
                        step_size = lr / (1 - beta1 ** state["step"])
                    buffered[2] = step_size
                if weight_decay != 0:
                    p_fp32.add_(p_fp32, alpha=-weight_decay * lr)
                if n_sma >= 5:
                    denom = exp_avg_sq.sqrt().add_(eps)
                    p_fp32.addcdiv_(exp_avg, denom, value=-step_size)
                else:
                    p_fp32.add_(exp_avg, alpha=-step_size)
                p.copy_(p_fp32)


class AdaBound(torch.optim.Optimizer):
    """torch_optimizer.AdaBound (0.1.0, Luo et al. 2019), ``amsbound=False``: Adam whose per-element step is clamped
    into bounds that converge to ``final_lr * lr / base_lr``; ``base_lrs`` are the group lrs at construction."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), final_lr=0.1, gamma=1e-3, eps=1e-8, weight_decay=0):
        if lr <= 0.0:
            raise ValueError(f"Invalid learning rate: {lr}")
        if eps < 0.0:
            raise ValueError(f"Invalid epsilon value: {eps}")
        if not 0.0 <= betas[0] < 1.0 or not 0.0 <= betas[1] < 1.0:
            raise ValueError(f"Invalid beta parameters: {betas}")
        defaults = dict(lr=lr, betas=betas, final_lr=final_lr, gamma=gamma, eps=eps, weight_decay=weight_decay)
        super().__init__(params, defaults)
        self.base_lrs = [group["lr"] for group in self.param_groups]

    @torch.no_grad()
    def step(self, closure=None):
        for group, base_lr in zip(self.param_groups, self.base_lrs):
            for p in group["params"]:
                if p.grad is None:
                    continue
                grad = p.grad
                state = self.state[p]
                if len(state) == 0:
                    state["step"] = 0
                    state["exp_avg"] = torch.zeros_like(p)
                    state["exp_avg_sq"] = torch.zeros_like(p)
                exp_avg, exp_avg_sq = state["exp_avg"], state["exp_avg_sq"]
                beta1, beta2 = group["betas"]
                state["step"] += 1
                if group["weight_decay"] != 0:
                    grad = grad.add(p, alpha=group["weight_decay"])
                exp_avg.mul_(beta1).add_(grad, alpha=1 - beta1)
                exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=1 - beta2)
                denom = exp_avg_sq.sqrt().add_(group["eps"])
                bias_correction1 = 1 - beta1 ** state["step"]
                bias_correction2 = 1 - beta2 ** state["step"]
                step_size = group["lr"] * math.sqrt(bias_correction2) / bias_correction1
                final_lr = group["final_lr"] * group["lr"] / base_lr
                lower_bound = final_lr * (1 - 1 / (group["gamma"] * state["step"] + 1))
                upper_bound = final_lr * (1 + 1 / (group["gamma"] * state["step"]))
                step_size = torch.full_like(denom, step_size)
                step_size.div_(denom).clamp_(lower_bound, upper_bound).mul_(exp_avg)
                p.add_(-step_size)


OPTIMIZERS = {"RAdam": RAdam, "AdaBound": AdaBound}
