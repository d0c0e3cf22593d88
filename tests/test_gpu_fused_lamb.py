"""GPU tests for the multi-tensor LAMB kernels (ops/hip/multi_tensor.hip) and
ops.FusedLamb: numerics vs the same formulas in float64, misaligned views,
edge cases, bitwise reproducibility, the torch oracle, no host sync, and a
single-peer hivemind_amd.Optimizer run.

Run on an MI355X via: python -m pytest tests/test_gpu_fused_lamb.py -m gpu -q
"""

import math

import pytest
import torch
import torch.nn as nn

pytestmark = [
    pytest.mark.gpu,
    pytest.mark.skipif(not torch.cuda.is_available(), reason="needs an MI355X"),
]

LR, BETA1, BETA2, EPS, WD = 1e-2, 0.9, 0.999, 1e-6, 0.01
TRUST_LO, TRUST_HI = 0.0, 10.0
STEP = 3
MAX_NORM = 1.0
# 2048*256+3 crosses the grid-stride wrap of the older multi-tensor kernels;
# 4096/4097 straddle one block's chunk; the 50 small tensors push n past MT_CHUNK
SIZES = [1, 7, 333, 4096, 4097, 64 * 1024 + 5, 2048 * 256 + 3] + [5] * 50
MIRRORED = (2, 5)


def _randn_params(n, gen):
    """Standard normal, clamped to |p| <= 3.5: a bf16 mirror is compared at
    atol=0.01, and bf16's rounding error (half an ulp) is 2^-7 = 0.0078 below
    |p| = 4 but 0.0156 above it. One step moves p by about 0.1 at the most."""
    return torch.randn(n, generator=gen).clamp_(-3.5, 3.5)


def _reference_step(params, grads, ms, vs, clip, wd=WD, lo=TRUST_LO, hi=TRUST_HI, lr=LR, step=STEP):
    """The LAMB formulas of ops.Lamb in float64 on the CPU, from the inputs as given."""
    out = []
    for p, g, m, v in zip(params, grads, ms, vs):
        p, g, m, v = (x.detach().cpu().double() for x in (p, g, m, v))
        g = clip * g
        m = BETA1 * m + (1 - BETA1) * g
        v = BETA2 * v + (1 - BETA2) * g * g
        u = (m / (1 - BETA1 ** step)) / ((v / (1 - BETA2 ** step)).sqrt() + EPS) + wd * p
        p_norm, u_norm = p.norm().item(), u.norm().item()
        trust = p_norm / u_norm if (p_norm > 0 and u_norm > 0) else 1.0
        trust = min(max(trust, lo), hi)
        out.append((p - lr * trust * u, m, v, trust))
    return out


def _reference_clip(grads, max_norm=MAX_NORM):
    total = math.sqrt(sum(g.detach().cpu().double().pow(2).sum().item() for g in grads))
    return total, min(1.0, max_norm / (total + 1e-6))


def _device_clip(grads, max_norm=MAX_NORM):
    from hivemind_amd.ops import hip_ops

    sumsq = torch.zeros(1, device="cuda")
    hip_ops().multi_grad_sumsq_(grads, sumsq)
    return sumsq, (max_norm / (sumsq.sqrt() + 1e-6)).clamp_(max=1.0)


def _check_against_reference(params, ms, vs, mirrors, trust, reference):
    trust = trust.cpu()
    for i, (p_ref, m_ref, v_ref, trust_ref) in enumerate(reference):
        p, m, v = params[i].cpu().double(), ms[i].cpu().double(), vs[i].cpu().double()
        assert torch.allclose(p, p_ref, atol=1e-5, rtol=1e-5), (i, (p - p_ref).abs().max())
        assert torch.allclose(m, m_ref, atol=1e-6, rtol=0), (i, (m - m_ref).abs().max())
        assert torch.allclose(v, v_ref, atol=1e-6, rtol=0), (i, (v - v_ref).abs().max())
        if mirrors[i] is not None:
            mirror = mirrors[i].cpu().double()
            assert torch.allclose(mirror, p_ref, atol=0.01, rtol=0), (i, (mirror - p_ref).abs().max())
        assert abs(trust[i].item() - trust_ref) <= 1e-4 * abs(trust_ref), (i, trust[i].item(), trust_ref)


@pytest.fixture(scope="module")
def case():
    """Inputs on the CPU (never modified) and their float64 reference, shared by
    the kernel and the reproducibility tests."""
    gen = torch.Generator().manual_seed(21)
    params = [_randn_params(s, gen) for s in SIZES]
    grads = [
        torch.randn(s, generator=gen).to(torch.bfloat16 if i % 2 else torch.float32)
        for i, s in enumerate(SIZES)
    ]
    ms = [torch.rand(s, generator=gen) * 0.1 for s in SIZES]
    vs = [torch.rand(s, generator=gen) * 0.1 for s in SIZES]
    total, clip = _reference_clip(grads)
    assert total > MAX_NORM, "clipping must be active"
    return dict(params=params, grads=grads, ms=ms, vs=vs, total=total, clip=clip,
                reference=_reference_step(params, grads, ms, vs, clip))


def _run_case(case):
    from hivemind_amd.ops import hip_ops

    params = [x.cuda() for x in case["params"]]
    grads = [x.cuda() for x in case["grads"]]
    ms = [x.cuda() for x in case["ms"]]
    vs = [x.cuda() for x in case["vs"]]
    mirrors = [torch.zeros(s, device="cuda", dtype=torch.bfloat16) if i in MIRRORED else None
               for i, s in enumerate(SIZES)]
    sumsq, clip = _device_clip(grads)
    trust = hip_ops().multi_lamb_(params, grads, ms, vs, mirrors, LR, BETA1, BETA2, EPS, WD, STEP,
                                  TRUST_LO, TRUST_HI, clip)
    torch.cuda.synchronize()
    return dict(params=params, grads=grads, ms=ms, vs=vs, mirrors=mirrors, trust=trust, sumsq=sumsq)


def test_multi_lamb_matches_float64_reference(case):
    out = _run_case(case)
    assert out["trust"].shape == (len(SIZES),) and out["trust"].dtype == torch.float32
    assert out["trust"].is_cuda
    # fp32 blocked summation of ~6e5 positive terms: far below 1e-4 relative
    assert abs(out["sumsq"].item() - case["total"] ** 2) <= 1e-4 * case["total"] ** 2
    _check_against_reference(out["params"], out["ms"], out["vs"], out["mirrors"], out["trust"],
                             case["reference"])
    for g, g0 in zip(out["grads"], case["grads"]):
        assert torch.equal(g.cpu(), g0), "the kernels must not write the gradients"


def test_multi_lamb_is_bitwise_reproducible(case):
    first, second = _run_case(case), _run_case(case)
    assert torch.equal(first["sumsq"], second["sumsq"])
    assert torch.equal(first["trust"], second["trust"])
    for key in ("params", "ms", "vs"):
        for a, b in zip(first[key], second[key]):
            assert torch.equal(a, b), key
    for a, b in zip(first["mirrors"], second["mirrors"]):
        assert (a is None and b is None) or torch.equal(a, b)


def _sliced(values, dtype, offset, sentinel=3.0):
    """values as the [offset:offset+n] slice of a flat sentinel-filled GPU buffer."""
    n = values.numel()
    backing = torch.full((n + offset + 1,), sentinel, dtype=dtype, device="cuda")
    view = backing[offset:offset + n]
    view.copy_(values)
    return backing, view


def test_multi_lamb_on_misaligned_views():
    """Every tensor is the [1:1+n] slice of a larger buffer, so no base pointer
    is 16-byte aligned (tensors 0 and 1: fp32 and bf16 grads, peeled head then
    vectors). Tensor 2 shifts m by one more element, so its pointers cannot be
    aligned together and it takes the scalar path. Nothing outside the slices
    may change."""
    from hivemind_amd.ops import hip_ops

    n = 4099
    gen = torch.Generator().manual_seed(22)
    grad_dtypes = [torch.float32, torch.bfloat16, torch.bfloat16]
    m_offsets = [1, 1, 2]
    backings, params, grads, ms, vs, mirrors = [], [], [], [], [], []
    for grad_dtype, m_offset in zip(grad_dtypes, m_offsets):
        for values, dtype, offset, dest in (
            (_randn_params(n, gen), torch.float32, 1, params),
            (torch.randn(n, generator=gen), grad_dtype, 1, grads),
            (torch.rand(n, generator=gen) * 0.1, torch.float32, m_offset, ms),
            (torch.rand(n, generator=gen) * 0.1, torch.float32, 1, vs),
            (torch.zeros(n), torch.bfloat16, 1, mirrors),
        ):
            backing, view = _sliced(values, dtype, offset)
            assert view.is_contiguous()
            backings.append((backing, offset, backing.clone()))
            dest.append(view)
    assert all(p.data_ptr() % 16 != 0 for p in params)
    inputs = [[x.clone() for x in xs] for xs in (params, grads, ms, vs)]
    total, clip_ref = _reference_clip(grads)
    assert total > MAX_NORM
    reference = _reference_step(*inputs, clip_ref)

    sumsq, clip = _device_clip(grads)
    trust = hip_ops().multi_lamb_(params, grads, ms, vs, mirrors, LR, BETA1, BETA2, EPS, WD, STEP,
                                  TRUST_LO, TRUST_HI, clip)
    torch.cuda.synchronize()
    assert abs(sumsq.item() - total ** 2) <= 1e-4 * total ** 2
    _check_against_reference(params, ms, vs, mirrors, trust, reference)
    for g, g0 in zip(grads, inputs[1]):
        assert torch.equal(g, g0)
    for backing, offset, before in backings:
        assert torch.equal(backing[:offset], before[:offset]), "wrote in front of a slice"
        assert torch.equal(backing[offset + n:], before[offset + n:]), "wrote past a slice"


def test_multi_lamb_edge_cases():
    from hivemind_amd.ops import hip_ops

    gen = torch.Generator().manual_seed(23)
    n = 300
    # [0] all-zero parameter -> trust 1;  [1] zero grad, zero state, wd=0 -> zero update, trust 1
    params = [torch.zeros(n, device="cuda"), torch.randn(n, generator=gen).cuda()]
    grads = [torch.randn(n, generator=gen).cuda(), torch.zeros(n, device="cuda")]
    ms = [torch.zeros(n, device="cuda") for _ in range(2)]
    vs = [torch.zeros(n, device="cuda") for _ in range(2)]
    before = [p.clone() for p in params]
    g0 = grads[0].clone()
    trust = hip_ops().multi_lamb_(params, grads, ms, vs, [None, None], 0.1, BETA1, BETA2, EPS, 0.0, 1,
                                  0.0, 10.0, None)
    assert trust.tolist() == [1.0, 1.0]
    assert torch.equal(params[1], before[1]) and torch.isfinite(params[1]).all()
    assert torch.equal(ms[1], torch.zeros_like(ms[1])) and torch.equal(vs[1], torch.zeros_like(vs[1]))
    # first step, wd=0, trust 1: p = -lr * g / (|g| + eps)
    expected = -0.1 * g0.double() / (g0.double().abs() + EPS)
    assert torch.allclose(params[0].double(), expected, atol=1e-5, rtol=1e-5)

    # ... then the clamp applies: the same zero parameter with trust clamped up to 2
    p2, m2, v2 = torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    trust = hip_ops().multi_lamb_([p2], [g0], [m2], [v2], [None], 0.1, BETA1, BETA2, EPS, 0.0, 1,
                                  2.0, 10.0, None)
    assert trust.tolist() == [2.0]
    assert torch.allclose(p2.double(), 2 * expected, atol=1e-5, rtol=1e-5)

    # weight_decay=0 with non-trivial state, against the float64 formulas
    params = [torch.randn(1000, generator=gen).cuda()]
    grads = [torch.randn(1000, generator=gen).cuda()]
    ms = [(torch.rand(1000, generator=gen) * 0.1).cuda()]
    vs = [(torch.rand(1000, generator=gen) * 0.1).cuda()]
    reference = _reference_step(params, grads, ms, vs, 1.0, wd=0.0)
    trust = hip_ops().multi_lamb_(params, grads, ms, vs, [None], LR, BETA1, BETA2, EPS, 0.0, STEP,
                                  TRUST_LO, TRUST_HI, None)
    _check_against_reference(params, ms, vs, [None], trust, reference)


def _oracle_pair(max_grad_norm):
    """FusedLamb and ClippingWrapper(Lamb) over clones of one small mixed list:
    two groups (one without weight decay), a size past one block's chunk."""
    from hivemind_amd.moe.server.layers.optim import ClippingWrapper
    from hivemind_amd.ops import FusedLamb, Lamb

    gen = torch.Generator().manual_seed(24)
    sizes = [1, 7, 333, 4097, 3 * 4096 + 11]
    init = [_randn_params(s, gen) for s in sizes]

    def groups():
        params = [nn.Parameter(x.clone().cuda()) for x in init]
        return params, [{"params": params[0::2], "weight_decay": 0.01},
                        {"params": params[1::2], "weight_decay": 0.0}]

    params_f, groups_f = groups()
    params_o, groups_o = groups()
    fused = FusedLamb(groups_f, lr=LR, max_grad_norm=max_grad_norm)
    oracle = ClippingWrapper(Lamb(groups_o, lr=LR), max_grad_norm)
    return gen, params_f, fused, params_o, oracle


def test_fused_lamb_matches_oracle_on_device():
    from hivemind_amd.ops import bind_grad

    gen, params_f, fused, params_o, oracle = _oracle_pair(0.5)
    mirror = torch.zeros_like(params_f[3], dtype=torch.bfloat16)
    fused.set_mirror(params_f[3], mirror)
    for _ in range(3):
        for i, (pf, po) in enumerate(zip(params_f, params_o)):
            g = torch.randn(pf.shape, generator=gen).to(torch.bfloat16 if i % 2 else torch.float32).cuda()
            bind_grad(pf, g.clone())
            # the oracle scales its grads in place, which would round bf16 ones again:
            # it gets the same values in fp32
            po.grad = g.float()
        assert torch.sqrt(sum(p.grad.double().pow(2).sum() for p in params_f)) > 0.5
        grads_before = [p.grad.clone() for p in params_f]
        fused.step()
        oracle.step()
        for i, (pf, po) in enumerate(zip(params_f, params_o)):
            assert torch.equal(pf.grad, grads_before[i])
            assert torch.allclose(pf, po, atol=1e-5, rtol=1e-5), (i, (pf - po).abs().max())
            sf, so = fused.state[pf], oracle.state[po]
            assert sf["step"] == so["step"]
            assert torch.allclose(sf["exp_avg"], so["exp_avg"], atol=1e-6, rtol=0), i
            assert torch.allclose(sf["exp_avg_sq"], so["exp_avg_sq"], atol=1e-6, rtol=0), i
    assert torch.allclose(mirror.float(), params_f[3], atol=0.01, rtol=0)
    assert all(r.is_cuda and r.dim() == 0 for r in fused.last_trust_ratios.values())
    assert set(fused.last_trust_ratios) == set(params_f)


def test_fused_lamb_step_does_not_sync():
    from hivemind_amd.ops import FusedLamb, Lamb

    gen = torch.Generator().manual_seed(25)

    def setup(cls, **kwargs):
        params = [nn.Parameter(torch.randn(s, generator=gen).cuda()) for s in (5, 4097)]
        opt = cls(params, lr=LR, **kwargs)
        for p in params:
            p.grad = torch.randn(p.shape, generator=gen).cuda()
        opt.step()  # warm-up: allocates the state
        return opt

    lamb = setup(Lamb)
    fused = setup(FusedLamb, max_grad_norm=1.0)
    torch.cuda.synchronize()
    previous = torch.cuda.get_sync_debug_mode()
    try:
        torch.cuda.set_sync_debug_mode("error")
        try:
            lamb.step()
            mode_works = False
        except RuntimeError:
            mode_works = True
        if mode_works:
            fused.step()  # raises if anything in it waits for the device
    finally:
        torch.cuda.set_sync_debug_mode(previous)
    if not mode_works:
        pytest.skip("sync debug mode does not flag Lamb.step() on this build")
    torch.cuda.synchronize()
    assert all(torch.isfinite(p).all() for group in fused.param_groups for p in group["params"])


def test_fused_lamb_in_collaborative_optimizer():
    """One peer, offloaded fp32 masters on the GPU stepped by FusedLamb, a tiny
    bf16 MLP as the live model."""
    from hivemind_amd import DHT, Optimizer
    from hivemind_amd.ops import FusedLamb

    torch.manual_seed(26)
    model = nn.Sequential(nn.Linear(16, 32), nn.Tanh(), nn.Linear(32, 1)).cuda().to(torch.bfloat16)
    X = torch.randn(64, 16, device="cuda", dtype=torch.bfloat16)
    y = X.float().sum(-1, keepdim=True)

    def fixed_batch_loss():
        with torch.no_grad():
            return (model(X).float() - y).pow(2).mean().item()

    dht = DHT(start=True)
    opt = Optimizer(
        dht=dht, run_id="fused_lamb_gpu", target_batch_size=8, batch_size_per_step=4,
        optimizer=lambda pg: FusedLamb(pg, lr=0.05, max_grad_norm=1.0),
        params=[{"params": list(model.parameters())}],
        offload_optimizer=True,
        matchmaking_time=0.5, averaging_timeout=20.0,
        tracker_opts=dict(min_refresh_period=0.1, default_refresh_period=0.2),
    )
    try:
        first = fixed_batch_loss()
        for _ in range(80):
            loss = (model(X).float() - y).pow(2).mean()
            loss.backward()
            opt.step()
            opt.zero_grad()
            if opt.local_epoch >= 6:
                break
        assert opt.local_epoch >= 3, opt.local_epoch
        inner = opt.state_averager.optimizer
        assert isinstance(inner, FusedLamb)
        assert inner.last_trust_ratios and all(r.is_cuda for r in inner.last_trust_ratios.values())
        assert all(torch.isfinite(p).all() for p in model.parameters())
        assert fixed_batch_loss() < first, (first, fixed_batch_loss())
    finally:
        opt.shutdown()
        dht.shutdown()
