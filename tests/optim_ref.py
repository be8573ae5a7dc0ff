"""float64 numpy restatement of one optimiser step as `csrc/pcc_optim.hip` defines it: `clip_grad_norm_` over the tensors that
have a gradient, then torch's default Adam (no amsgrad, no weight decay) or SGD with momentum (`optim.SGD(momentum=0.9)`).
tests/test_cpu_optim_ref.py holds it against CPU float64 torch.  Nothing here imports the package under test."""
import numpy as np


def total_norm(grads):
    """sqrt of the sum of squares over every gradient that is not None."""
    return float(np.sqrt(sum(float(np.sum(np.asarray(g, np.float64) ** 2)) for g in grads if g is not None)))


def clip_coef(norm, max_norm):
    """`clip_grad_norm_`: min(1, max_norm / (norm + 1e-6)); None / <= 0: no clipping.  A NaN norm gives NaN."""
    if max_norm is None or max_norm <= 0:
        return 1.0
    c = max_norm / (norm + 1e-6)
    if np.isnan(c):
        return c
    return min(1.0, c)


class State:
    """Per tensor: step count, first and second state (None until the tensor's first step)."""

    def __init__(self, n):
        self.step = [0] * n
        self.s1 = [None] * n
        self.s2 = [None] * n


def step(params, grads, state, lr, mode="adam", betas=(0.9, 0.999), eps=1e-8, momentum=0.9, max_norm=None):
    """Updates params (list of float64 arrays) and state in place; a tensor whose gradient is None is left alone.
    Returns the total norm (None without clipping)."""
    norm = total_norm(grads) if max_norm is not None and max_norm > 0 else None
    coef = clip_coef(norm, max_norm)
    b1, b2 = betas
    for i, (p, g) in enumerate(zip(params, grads)):
        if g is None:
            continue
        g = np.asarray(g, np.float64) * coef
        state.step[i] += 1
        t = state.step[i]
        if mode == "adam":
            if state.s1[i] is None:
                state.s1[i], state.s2[i] = np.zeros_like(p), np.zeros_like(p)
            state.s1[i] = b1 * state.s1[i] + (1 - b1) * g
            state.s2[i] = b2 * state.s2[i] + (1 - b2) * g * g
            p -= (lr / (1 - b1 ** t)) * state.s1[i] / (np.sqrt(state.s2[i]) / np.sqrt(1 - b2 ** t) + eps)
        elif mode == "sgd":
            state.s1[i] = g.copy() if state.s1[i] is None else momentum * state.s1[i] + g
            p -= lr * state.s1[i]
        else:
            raise ValueError(mode)
    return norm
