"""FusedLamb on the CPU (torch path): the mathematics must be that of
ClippingWrapper(Lamb, max_grad_norm) -- or plain Lamb without clipping -- with
the gradients left untouched, and its state dict must interchange with Lamb's."""

import copy

import pytest
import torch

from hivemind_amd.moe.server.layers.optim import ClippingWrapper
from hivemind_amd.ops import FusedLamb, Lamb

SIZES = [1, 7, 333, 4097]
HYPER = dict(lr=1e-2, betas=(0.9, 0.999), eps=1e-6)


def _make_groups(seed):
    """Two param groups over SIZES; the second one has weight_decay=0."""
    gen = torch.Generator().manual_seed(seed)
    params = [torch.nn.Parameter(torch.randn(s, generator=gen)) for s in SIZES]
    groups = [
        {"params": params[0::2], "weight_decay": 0.01},
        {"params": params[1::2], "weight_decay": 0.0},
    ]
    return params, groups


@pytest.mark.parametrize("max_grad_norm", [0.5, None])
def test_matches_clipped_lamb_oracle(max_grad_norm):
    params_f, groups_f = _make_groups(0)
    params_o, groups_o = _make_groups(0)
    fused = FusedLamb(groups_f, max_grad_norm=max_grad_norm, **HYPER)
    oracle = Lamb(groups_o, **HYPER)
    if max_grad_norm is not None:
        oracle = ClippingWrapper(oracle, max_grad_norm)

    gen = torch.Generator().manual_seed(1)
    for _ in range(3):
        grads = [torch.randn(p.shape, generator=gen) for p in params_f]
        global_norm = torch.sqrt(sum(g.double().pow(2).sum() for g in grads))
        assert global_norm > 0.5, "the clip must be active for this test to mean anything"
        for pf, po, g in zip(params_f, params_o, grads):
            pf.grad = g.clone()
            po.grad = g.clone()
        fused.step()
        oracle.step()
        for pf, g in zip(params_f, grads):
            assert torch.equal(pf.grad, g), "FusedLamb must not touch the gradients"
        for i, (pf, po) in enumerate(zip(params_f, params_o)):
            assert torch.allclose(pf, po, atol=1e-6), (i, (pf - po).abs().max())
            sf, so = fused.state[pf], oracle.state[po]
            assert sf["step"] == so["step"]
            assert torch.allclose(sf["exp_avg"], so["exp_avg"], atol=1e-6), i
            assert torch.allclose(sf["exp_avg_sq"], so["exp_avg_sq"], atol=1e-6), i
    assert set(fused.last_trust_ratios) == set(params_f)
    assert all(r.dim() == 0 for r in fused.last_trust_ratios.values())


def test_zero_parameter_gets_unit_trust_then_clamp():
    grad = torch.randn(50, generator=torch.Generator().manual_seed(2))
    # trust = 1 (||p|| = 0) inside the clamp range
    p = torch.nn.Parameter(torch.zeros(50))
    opt = FusedLamb([p], lr=0.1, weight_decay=0.0, clamp_trust_ratio=(0.0, 10.0))
    p.grad = grad.clone()
    opt.step()
    assert opt.last_trust_ratios[p].item() == 1.0
    # first step, wd=0: update = g / (|g| + eps), so p = -lr * 1 * sign(g) up to eps
    assert torch.allclose(p.detach(), -0.1 * torch.sign(grad), atol=1e-4)
    # ... and the clamp applies after that
    q = torch.nn.Parameter(torch.zeros(50))
    opt = FusedLamb([q], lr=0.1, weight_decay=0.0, clamp_trust_ratio=(2.0, 10.0))
    q.grad = grad.clone()
    opt.step()
    assert opt.last_trust_ratios[q].item() == 2.0
    assert torch.allclose(q.detach(), 2 * p.detach(), atol=1e-6)


def test_zero_update_leaves_parameter_unchanged():
    before = torch.randn(33, generator=torch.Generator().manual_seed(3))
    for max_grad_norm in (None, 1.0):
        p = torch.nn.Parameter(before.clone())
        opt = FusedLamb([p], lr=0.1, weight_decay=0.0, max_grad_norm=max_grad_norm)
        p.grad = torch.zeros(33)
        opt.step()
        assert opt.last_trust_ratios[p].item() == 1.0
        assert torch.isfinite(p).all()
        assert torch.equal(p.detach(), before)


def test_state_dict_interchanges_with_lamb():
    params_l, groups_l = _make_groups(4)
    params_f, groups_f = _make_groups(4)
    lamb = Lamb(groups_l, **HYPER)
    fused = FusedLamb(groups_f, **HYPER)
    gen = torch.Generator().manual_seed(5)
    for _ in range(2):
        for p in params_l:
            p.grad = torch.randn(p.shape, generator=gen)
        lamb.step()
    # deep copy, as a checkpoint would be: load_state_dict keeps references to same-dtype tensors
    fused.load_state_dict(copy.deepcopy(lamb.state_dict()))
    with torch.no_grad():
        for pf, pl in zip(params_f, params_l):
            pf.copy_(pl)
    for pf, pl in zip(params_f, params_l):
        g = torch.randn(pl.shape, generator=gen)
        pl.grad, pf.grad = g.clone(), g.clone()
    lamb.step()
    fused.step()
    for pf, pl in zip(params_f, params_l):
        assert fused.state[pf]["step"] == 3
        # equal up to the oracle test's tolerance: Lamb scales by lr * trust in
        # float64 on the host, FusedLamb in float32 on the device
        assert torch.allclose(pf, pl, atol=1e-6), (pf - pl).abs().max()

    # and back: FusedLamb's state loads into Lamb
    params_b, groups_b = _make_groups(4)
    back = Lamb(groups_b, **HYPER)
    back.load_state_dict(copy.deepcopy(fused.state_dict()))
    for pb, pf in zip(params_b, params_f):
        assert back.state[pb]["step"] == 3
        assert torch.equal(back.state[pb]["exp_avg"], fused.state[pf]["exp_avg"])
        assert torch.equal(back.state[pb]["exp_avg_sq"], fused.state[pf]["exp_avg_sq"])


def test_albert_trainer_fused_lamb_choice(tmp_path):
    """`run_trainer.py --optimizer fused_lamb` builds FusedLamb with the recipe's
    clipping and trains through hivemind_amd.Optimizer: 1-peer swarm, tiny
    shapes, 2 epochs (the twin of test_albert_trainer_lamb_recipe_smoke)."""
    import os
    import subprocess
    import sys

    proc = subprocess.run(
        [
            sys.executable, "examples/albert/run_trainer.py",
            "--optimizer", "fused_lamb", "--clip_grad_norm", "1.0",
            "--batch_size", "4", "--seq_len", "32", "--target_batch_size", "8",
            "--max_epochs", "2", "--state_path", str(tmp_path / "state.pt"),
            "--backup_every_epochs", "0",
        ],
        capture_output=True, text=True, timeout=420,
        cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
    )
    assert proc.returncode == 0, f"trainer failed:\n{proc.stderr[-2000:]}"
    assert "epoch 2" in proc.stderr or "epoch 2" in proc.stdout, proc.stderr[-1500:]
