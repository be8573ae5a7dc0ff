"""tests/optim_ref.py (the float64 reference of the optimiser kernels) against CPU float64 `torch.optim.Adam` / `SGD` with
`clip_grad_norm_`: parameters, state and the reported norm to 1e-12 over 5 steps."""
import numpy as np
import pytest
import torch

from tests import optim_ref as R

SIZES = (1, 3, 7, 0, 257, 40)
SKIP = 2                                  # this tensor has no gradient on the odd steps


def _grads(rng, step, scale):
    return [None if (i == SKIP and step % 2 == 1) else rng.standard_normal(n) * scale for i, n in enumerate(SIZES)]


@pytest.mark.parametrize("mode", ["adam", "sgd"])
@pytest.mark.parametrize("max_norm,scale", [(1.0, 3.0), (1.0, 1e-3), (None, 1.0)])     # clip active, inactive, absent
def test_reference_matches_float64_torch(mode, max_norm, scale):
    rng = np.random.default_rng(11)
    p0 = [rng.standard_normal(n) for n in SIZES]
    tp = [torch.tensor(p, dtype=torch.float64, requires_grad=True) for p in p0]
    opt = torch.optim.Adam(tp, lr=1e-2) if mode == "adam" else torch.optim.SGD(tp, lr=1e-2, momentum=0.9)
    sched = torch.optim.lr_scheduler.StepLR(opt, step_size=2, gamma=0.5)
    params, state = [p.copy() for p in p0], R.State(len(SIZES))
    for s in range(5):
        grads = _grads(rng, s, scale)
        for p, g in zip(tp, grads):
            p.grad = None if g is None else torch.from_numpy(g.copy())
        lr = opt.param_groups[0]["lr"]
        if max_norm is not None:
            norm_t = float(torch.nn.utils.clip_grad_norm_(tp, max_norm))
        opt.step()
        sched.step()
        norm = R.step(params, grads, state, lr, mode=mode, max_norm=max_norm)
        if max_norm is not None:
            assert abs(norm - norm_t) <= 1e-12 * max(1.0, norm_t)
        else:
            assert norm is None
        for i, (p, q) in enumerate(zip(params, tp)):
            assert np.abs(p - q.detach().numpy()).max(initial=0.0) <= 1e-12, (s, i)
            st = opt.state.get(q, {})
            if mode == "adam" and st:
                assert int(st["step"]) == state.step[i]
                assert np.abs(state.s1[i] - st["exp_avg"].numpy()).max(initial=0.0) <= 1e-12
                assert np.abs(state.s2[i] - st["exp_avg_sq"].numpy()).max(initial=0.0) <= 1e-12
            if mode == "sgd" and st:
                assert np.abs(state.s1[i] - st["momentum_buffer"].numpy()).max(initial=0.0) <= 1e-12
    assert state.step[SKIP] == 3 and state.step[0] == 5


def test_clip_coefficient_rule():
    assert R.clip_coef(0.5, 1.0) == 1.0 and R.clip_coef(4.0, 1.0) == 1.0 / (4.0 + 1e-6)
    assert R.clip_coef(4.0, None) == 1.0 and R.clip_coef(4.0, 0.0) == 1.0
    assert np.isnan(R.clip_coef(float("nan"), 1.0)) and R.clip_coef(float("inf"), 1.0) == 0.0
