"""hivemind_amd.ops: hand-written CDNA4 HIP kernels + torch reference impls.

GPU tensors dispatch to the in-tree ``hivemind_amd._hip_ops`` extension
(built by setup.py with PYTORCH_ROCM_ARCH=gfx950). If a GPU tensor arrives
and the extension is missing, ops raise immediately -- there is no silent
eager fallback on the GPU path. CPU tensors use the torch reference
implementations (which are also the numerics oracle for the GPU tests).
"""

from __future__ import annotations

import os
from typing import Optional, Tuple

import torch

from ..utils.logging import get_logger

logger = get_logger(__name__)

_hip_ops = None
_hip_import_error: Optional[BaseException] = None
try:
    from hivemind_amd import _hip_ops  # type: ignore[no-redef]
except BaseException as e:  # pragma: no cover
    _hip_import_error = e


def hip_ops():
    """The extension module; raises loudly if unavailable (never silently falls back)."""
    if _hip_ops is None:
        raise RuntimeError(
            "hivemind_amd._hip_ops extension is not built -- run "
            "`PYTORCH_ROCM_ARCH=gfx950 python setup.py build_ext --inplace` "
            f"(import error: {_hip_import_error!r})"
        )
    return _hip_ops


def hip_available() -> bool:
    return _hip_ops is not None


def bind_grad(param: torch.Tensor, grad: torch.Tensor) -> None:
    """Assign a gradient buffer whose dtype may differ from the parameter's
    (e.g. bf16 swarm-averaged grads bound to fp32 master params; the fused
    AdamW kernel consumes bf16 grads directly). torch >= 2.10 enforces
    grad-dtype matching unless grad_dtype is relaxed first."""
    if grad is not None and grad.dtype != param.dtype:
        try:
            param.grad_dtype = None
        except (AttributeError, RuntimeError):
            grad = grad.to(param.dtype)
    param.grad = grad


# ---------------------------------------------------------------------------
# fused layernorm (optionally fused residual add)
# ---------------------------------------------------------------------------


class _FusedLayerNorm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, residual, gamma, beta, eps):
        outs = hip_ops().layernorm_fwd(x.contiguous(), residual.contiguous() if residual is not None else None,
                                       gamma.contiguous(), beta.contiguous(), eps)
        if residual is not None:
            y, mean, rstd, h = outs
        else:
            y, mean, rstd = outs
            h = x.detach()
        ctx.save_for_backward(h, gamma, mean, rstd)
        ctx.has_residual = residual is not None
        return y

    @staticmethod
    def backward(ctx, dy):
        h, gamma, mean, rstd = ctx.saved_tensors
        dx, dgamma, dbeta = hip_ops().layernorm_bwd(dy.contiguous(), h.contiguous(), gamma, mean, rstd)
        # d(x) and d(residual) are identical for the fused residual add
        dres = dx if ctx.has_residual else None
        return dx, dres, dgamma.to(gamma.dtype), dbeta.to(gamma.dtype), None


def fused_layernorm(
    x: torch.Tensor,
    gamma: torch.Tensor,
    beta: torch.Tensor,
    residual: Optional[torch.Tensor] = None,
    eps: float = 1e-12,
) -> torch.Tensor:
    """y = LayerNorm(x + residual), one fused HIP kernel (wave-per-row, bf16)
    on GPU; torch reference on CPU."""
    if x.is_cuda and x.dtype == torch.bfloat16:
        return _FusedLayerNorm.apply(x, residual, gamma, beta, eps)
    h = x + residual if residual is not None else x
    return torch.nn.functional.layer_norm(h.float(), (h.shape[-1],), gamma.float(), beta.float(), eps).to(x.dtype)


class _FusedBiasGelu(torch.autograd.Function):
    """Forward writes only gelu(x + bias); backward recomputes x + bias from
    the saved input (x is retained by autograd for the producing GEMM's
    backward anyway), so no pre-activation tensor is ever materialized."""

    @staticmethod
    def forward(ctx, x, bias):
        x, bias = x.contiguous(), bias.contiguous()
        (out,) = hip_ops().bias_gelu_fwd(x, bias, False)
        ctx.save_for_backward(x, bias)
        ctx.bias_dtype = bias.dtype
        return out

    @staticmethod
    def backward(ctx, dy):
        x, bias = ctx.saved_tensors
        dx, dbias = hip_ops().bias_gelu_bwd_xb(dy.contiguous(), x, bias)
        return dx, dbias.to(ctx.bias_dtype)


def fused_bias_gelu(x: torch.Tensor, bias: torch.Tensor) -> torch.Tensor:
    """gelu_tanh(x + bias) -- the reference's gelu_fast (layers/common.py:10-16)."""
    if x.is_cuda and x.dtype == torch.bfloat16:
        return _FusedBiasGelu.apply(x, bias)
    return torch.nn.functional.gelu((x.float() + bias.float()), approximate="tanh").to(x.dtype)


class _FusedCrossEntropy(torch.autograd.Function):
    """Masked-LM cross-entropy that never materializes the [N, V] log-softmax:
    forward saves only the per-row logsumexp (fp32 [N]); backward recomputes
    softmax from the bf16 logits in one streaming pass. The mean is taken over
    rows with label != ignore_index, matching F.cross_entropy(ignore_index=-100).
    All reductions stay on device -- no host sync in either direction."""

    @staticmethod
    def forward(ctx, logits, labels):
        loss_sum, valid, lse = hip_ops().cross_entropy_fwd(logits.contiguous(), labels.contiguous())
        ctx.save_for_backward(logits, labels, lse, valid)
        return loss_sum / valid.clamp_min(1).to(torch.float32)

    @staticmethod
    def backward(ctx, dloss):
        logits, labels, lse, valid = ctx.saved_tensors
        dlogits = hip_ops().cross_entropy_bwd(
            logits.contiguous(), labels.contiguous(), lse,
            dloss.reshape(()).to(torch.float32).contiguous(), valid,
        )
        return dlogits, None


def fused_cross_entropy(logits: torch.Tensor, labels: torch.Tensor) -> torch.Tensor:
    """Mean cross-entropy over labels != -100 (the MLM loss of the ALBERT
    example). GPU bf16 path runs the fused kernels; everything else falls back
    to F.cross_entropy in fp32."""
    if logits.is_cuda and logits.dtype == torch.bfloat16 and logits.dim() == 2:
        return _FusedCrossEntropy.apply(logits, labels)
    return torch.nn.functional.cross_entropy(logits.float(), labels, ignore_index=-100)


# ---------------------------------------------------------------------------
# hand-written MFMA GEMM (guide §5 structure): x @ W^T with fused bias+GELU
# ---------------------------------------------------------------------------


def _mfma_shapes_ok(M: int, N: int, K: int) -> bool:
    return N % 128 == 0 and K % 32 == 0 and M >= 128 and N >= 128 and K >= 32


def mfma_matmul(x: torch.Tensor, weight: torch.Tensor) -> torch.Tensor:
    """Plain C = x @ weight^T through the hand-written MFMA kernel (pads M to 128)."""
    K = x.shape[-1]
    M = x.numel() // K
    N = weight.shape[0]
    assert _mfma_shapes_ok(M, N, K), (M, N, K)
    pad = (-M) % 128
    flat = x.reshape(M, K)
    if pad:
        flat = torch.nn.functional.pad(flat, (0, 0, 0, pad))
    (out,) = hip_ops().mfma_linear_bf16(flat.contiguous(), weight.contiguous(), None, False, False)
    out = out[:M]
    return out.reshape(*x.shape[:-1], N)


class _MfmaLinearGelu(torch.autograd.Function):
    """Forward: one MFMA kernel computing gelu(x @ W^T + b) with the pre-activation
    saved in the same pass (no separate bias/act memory round-trips).
    Backward: dact via the fused bias-gelu backward kernel, then two rocBLAS
    GEMMs for dx and dW (library GEMMs per the build rules)."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        K = x.shape[-1]
        M = x.numel() // K
        pad = (-M) % 128
        flat = x.reshape(M, K).contiguous()
        padded = torch.nn.functional.pad(flat, (0, 0, 0, pad)) if pad else flat
        out, pre_act = hip_ops().mfma_linear_bf16(padded, weight.contiguous(), bias.contiguous(), True, True)
        ctx.save_for_backward(flat, weight, pre_act)
        ctx.pad, ctx.M = pad, M
        ctx.x_shape = x.shape
        out = out[:M].reshape(*x.shape[:-1], weight.shape[0])
        return out

    @staticmethod
    def backward(ctx, dy):
        flat, weight, pre_act = ctx.saved_tensors
        M, pad = ctx.M, ctx.pad
        N = weight.shape[0]
        dy_flat = dy.reshape(M, N)
        if pad:
            dy_flat = torch.nn.functional.pad(dy_flat, (0, 0, 0, pad))
        dact, dbias = hip_ops().bias_gelu_bwd(dy_flat.contiguous(), pre_act)
        dact = dact[:M]
        dx = dact @ weight  # rocBLAS
        dweight = dact.t() @ flat  # rocBLAS
        return dx.reshape(ctx.x_shape), dweight, dbias.to(weight.dtype)


def fused_linear_gelu(x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor) -> torch.Tensor:
    """gelu(x @ W^T + b): MFMA kernel with fused epilogue on GPU; torch on CPU
    or for shapes the kernel doesn't cover."""
    K = x.shape[-1]
    M = x.numel() // K
    N = weight.shape[0]
    if x.is_cuda and x.dtype == torch.bfloat16 and _mfma_shapes_ok(M, N, K):
        return _MfmaLinearGelu.apply(x, weight, bias)
    return fused_bias_gelu(torch.nn.functional.linear(x, weight), bias)


# ---------------------------------------------------------------------------
# Llama-family fused ops: RMSNorm, SwiGLU, RoPE
# ---------------------------------------------------------------------------


class _FusedRMSNorm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, gamma, eps):
        y, rstd = hip_ops().rmsnorm_fwd(x.contiguous(), gamma.contiguous(), eps)
        ctx.save_for_backward(x, gamma, rstd)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, gamma, rstd = ctx.saved_tensors
        dx, dgamma = hip_ops().rmsnorm_bwd(dy.contiguous(), x.contiguous(), gamma, rstd)
        return dx, dgamma.to(gamma.dtype), None


def fused_rmsnorm(x: torch.Tensor, gamma: torch.Tensor, eps: float = 1e-5) -> torch.Tensor:
    """y = x * gamma / sqrt(mean(x^2) + eps), one HIP kernel on GPU."""
    if x.is_cuda and x.dtype == torch.bfloat16:
        return _FusedRMSNorm.apply(x, gamma, eps)
    xf = x.float()
    rstd = torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + eps)
    return (xf * rstd * gamma.float()).to(x.dtype)


class _FusedSwiGLU(torch.autograd.Function):
    @staticmethod
    def forward(ctx, gate, up):
        ctx.save_for_backward(gate, up)
        return hip_ops().swiglu_fwd(gate.contiguous(), up.contiguous())

    @staticmethod
    def backward(ctx, dy):
        gate, up = ctx.saved_tensors
        dgate, dup = hip_ops().swiglu_bwd(dy.contiguous(), gate.contiguous(), up.contiguous())
        return dgate, dup


def fused_swiglu(gate: torch.Tensor, up: torch.Tensor) -> torch.Tensor:
    """silu(gate) * up -- the Llama MLP activation, fused."""
    if gate.is_cuda and gate.dtype == torch.bfloat16:
        return _FusedSwiGLU.apply(gate, up)
    return torch.nn.functional.silu(gate.float()).mul(up.float()).to(gate.dtype)


class _FusedRoPE(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, cos_table, sin_table):
        ctx.save_for_backward(cos_table, sin_table)
        return hip_ops().rope_apply(x.contiguous(), cos_table, sin_table, 1.0)

    @staticmethod
    def backward(ctx, dy):
        cos_table, sin_table = ctx.saved_tensors
        return hip_ops().rope_apply(dy.contiguous(), cos_table, sin_table, -1.0), None, None


def fused_rope(x: torch.Tensor, cos_table: torch.Tensor, sin_table: torch.Tensor) -> torch.Tensor:
    """Rotate-half RoPE with host-precomputed fp32 cos/sin tables [tokens, head_dim/2].

    x: [..., tokens, heads, head_dim] flattened so that the trailing dims are
    (heads, head_dim) and tokens iterate over everything before them.
    """
    if x.is_cuda and x.dtype == torch.bfloat16:
        return _FusedRoPE.apply(x, cos_table, sin_table)
    half = x.shape[-1] // 2
    x1, x2 = x[..., :half].float(), x[..., half:].float()
    shape = [1] * (x.ndim - 3) + [cos_table.shape[0], 1, half]
    cos = cos_table.reshape(shape)
    sin = sin_table.reshape(shape)
    out1 = x1 * cos - x2 * sin
    out2 = x2 * cos + x1 * sin
    return torch.cat([out1, out2], dim=-1).to(x.dtype)


def build_rope_tables(seq_len: int, head_dim: int, base: float = 500000.0, device="cpu"):
    """Host-precomputed RoPE tables (guide: never compute trig on-device)."""
    half = head_dim // 2
    inv_freq = 1.0 / (base ** (torch.arange(0, half, dtype=torch.float32) / half))
    t = torch.arange(seq_len, dtype=torch.float32)
    freqs = torch.outer(t, inv_freq)  # [seq_len, half]
    return freqs.cos().to(device), freqs.sin().to(device)


# ---------------------------------------------------------------------------
# flash attention: hand-written CDNA4 kernels replacing AOTriton
# ---------------------------------------------------------------------------


class _FlashAttention(torch.autograd.Function):
    """bf16 flash attention on the hand-written CDNA4 kernels
    (ops/hip/flash_attention.hip). Forward saves O + logsumexp; backward runs
    the delta pre-pass and the two-kernel (dkdv, dq) split."""

    @staticmethod
    def forward(ctx, q, k, v, causal, scale):
        o, lse = hip_ops().flash_attn_fwd(q, k, v, causal, scale)
        ctx.save_for_backward(q, k, v, o, lse)
        ctx.causal, ctx.scale = causal, scale
        return o

    @staticmethod
    def backward(ctx, d_out):
        q, k, v, o, lse = ctx.saved_tensors
        dq, dk, dv = hip_ops().flash_attn_bwd(d_out, q, k, v, o, lse, ctx.causal, ctx.scale)
        return dq, dk, dv, None, None


def flash_attention_usable(q: torch.Tensor, k: torch.Tensor) -> bool:
    """True if the CDNA4 flash kernels handle these shapes: CUDA bf16
    [B, H, S, D] with D in {64, 128} and S % 64 == 0."""
    return (
        q.is_cuda
        and hip_available()
        and q.dtype == torch.bfloat16
        and q.shape[-1] in (64, 128)
        and q.shape[-2] % 64 == 0
        and k.shape[-2] == q.shape[-2]
    )


def flash_attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor,
                    causal: bool = False, scale: Optional[float] = None) -> torch.Tensor:
    """[B, H, S, D] attention. CUDA tensors run the hand-written CDNA4 flash
    kernels; CPU tensors use the torch reference (the numerics oracle).
    Backward requires H == Hkv -- expand grouped kv heads first."""
    if scale is None:
        scale = q.shape[-1] ** -0.5
    if q.is_cuda:
        # strided [B,H,S,D] views (e.g. the model's qkv-GEMM slices) feed the
        # kernels directly; the binding falls back to .contiguous() only when
        # the last dim is non-contiguous or rows are misaligned
        return _FlashAttention.apply(q, k, v, causal, float(scale))
    return torch.nn.functional.scaled_dot_product_attention(q, k, v, is_causal=causal, scale=scale)


# ---------------------------------------------------------------------------
# averaging primitives
# ---------------------------------------------------------------------------


@torch.no_grad()
def apply_delta_(tensor: torch.Tensor, delta: torch.Tensor, alpha: float = 1.0):
    """tensor += alpha * delta."""
    if (
        tensor.is_cuda
        and delta.device == tensor.device  # never hand the kernel a host pointer
        and tensor.dtype == delta.dtype
        and tensor.dtype in (torch.bfloat16, torch.float32)
    ):
        hip_ops().apply_delta_(tensor, delta.contiguous(), float(alpha))
    else:
        tensor.add_(delta.to(tensor.device, tensor.dtype), alpha=alpha)
    return tensor


@torch.no_grad()
def weighted_accumulate_(acc: torch.Tensor, x: torch.Tensor, w: float = 1.0):
    """acc += w * x."""
    if (
        acc.is_cuda
        and x.device == acc.device  # never hand the kernel a host pointer
        and acc.dtype == torch.float32
        and x.dtype in (torch.float32, torch.bfloat16)
    ):
        hip_ops().weighted_accumulate_(acc, x.contiguous(), float(w))
    else:
        acc.add_(x.to(acc.device, acc.dtype), alpha=w)
    return acc


# ---------------------------------------------------------------------------
# codecs (GPU fast path used by the compression layer)
# ---------------------------------------------------------------------------


@torch.no_grad()
def compress_fp16(t: torch.Tensor) -> torch.Tensor:
    if t.is_cuda:
        return hip_ops().compress_fp16(t.contiguous())
    return t.float().clamp_(-65504.0, 65504.0).half()


@torch.no_grad()
def decompress_fp16(t: torch.Tensor) -> torch.Tensor:
    if t.is_cuda:
        return hip_ops().decompress_fp16(t.contiguous())
    return t.float()


@torch.no_grad()
def quantize_blockwise(t: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """(int8 codes, per-4096-block absmax) -- SURVEY K7."""
    if t.is_cuda:
        q, absmax = hip_ops().quantize_blockwise(t.contiguous())
        return q, absmax
    flat = t.detach().float().flatten()
    n = flat.numel()
    blocks = (n + 4095) // 4096
    padded = torch.zeros(blocks * 4096)
    padded[:n] = flat
    view = padded.view(blocks, 4096)
    absmax = view.abs().amax(1)
    scale = torch.clamp_min(absmax / 127.0, torch.finfo(torch.float32).eps)
    q = torch.round(view / scale.unsqueeze(1)).clamp_(-127, 127).to(torch.int8).flatten()[:n]
    return q, absmax


@torch.no_grad()
def dequantize_blockwise(q: torch.Tensor, absmax: torch.Tensor) -> torch.Tensor:
    if q.is_cuda:
        return hip_ops().dequantize_blockwise(q.contiguous(), absmax.contiguous())
    n = q.numel()
    idx = torch.arange(n) // 4096
    return q.float() * (absmax[idx] / 127.0)


# ---------------------------------------------------------------------------
# fused AdamW
# ---------------------------------------------------------------------------


class Lamb(torch.optim.Optimizer):
    """LAMB (You et al.): Adam statistics + layer-wise trust-ratio scaling --
    the optimizer of the reference's collaborative ALBERT recipe
    (examples/albert/run_trainer.py LAMB + clipping). Runs on fp32 masters with
    an optional bf16 mirror like FusedAdamW; norms and the update run as torch
    (rocBLAS) ops on-device.
    """

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-6, weight_decay=0.01,
                 clamp_trust_ratio=(0.0, 10.0), mirrors=None):
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)
        super().__init__(params, defaults)
        self.clamp_trust_ratio = clamp_trust_ratio
        self._mirrors = mirrors or {}

    def set_mirror(self, param: torch.Tensor, mirror: torch.Tensor):
        self._mirrors[param] = mirror

    @torch.no_grad()
    def step(self, closure=None):
        loss = closure() if closure is not None else None
        for group in self.param_groups:
            beta1, beta2 = group["betas"]
            for p in group["params"]:
                if p.grad is None:
                    continue
                g = p.grad.float()
                state = self.state[p]
                if len(state) == 0:
                    state["step"] = 0
                    state["exp_avg"] = torch.zeros_like(p, dtype=torch.float32)
                    state["exp_avg_sq"] = torch.zeros_like(p, dtype=torch.float32)
                state["step"] += 1
                m, v = state["exp_avg"], state["exp_avg_sq"]
                m.mul_(beta1).add_(g, alpha=1 - beta1)
                v.mul_(beta2).addcmul_(g, g, value=1 - beta2)
                m_hat = m / (1 - beta1 ** state["step"])
                v_hat = v / (1 - beta2 ** state["step"])
                update = m_hat / (v_hat.sqrt() + group["eps"])
                if group["weight_decay"]:
                    update = update + group["weight_decay"] * p.float()
                p_norm = p.detach().float().norm()
                u_norm = update.norm()
                trust_ratio = torch.where(
                    (p_norm > 0) & (u_norm > 0), p_norm / u_norm, torch.ones_like(p_norm)
                ).clamp(*self.clamp_trust_ratio)
                p.data.add_(update.to(p.dtype), alpha=-group["lr"] * float(trust_ratio))
                mirror = self._mirrors.get(p)
                if mirror is not None:
                    mirror.copy_(p.data.to(mirror.dtype))
        return loss


class FusedLamb(torch.optim.Optimizer):
    """LAMB with optional global grad-norm clipping whose step never waits for
    the device: the mathematics of ``ClippingWrapper(Lamb(...), max_grad_norm)``
    (plain ``Lamb`` when ``max_grad_norm`` is None), except that gradients are
    left unscaled -- the clip coefficient stays on the device and is applied as
    the kernels load ``g``.

    CUDA fp32 contiguous params with fp32/bf16 contiguous grads run the
    multi-tensor HIP kernels (ops/hip/multi_tensor.hip): one launch sequence per
    (group, step-count) bucket, per-tensor trust ratios reduced on the device.
    Everything else (CPU tensors included) takes a torch path with the same
    formulas and no host read either. State keys match ``Lamb``, so state dicts
    interchange. ``last_trust_ratios`` maps param -> 0-dim tensor for logging.
    """

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-6, weight_decay=0.01,
                 clamp_trust_ratio=(0.0, 10.0), max_grad_norm=None, mirrors=None):
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)
        super().__init__(params, defaults)
        self.clamp_trust_ratio = clamp_trust_ratio
        self.max_grad_norm = max_grad_norm
        self._mirrors = mirrors or {}
        self.last_trust_ratios = {}

    def set_mirror(self, param: torch.Tensor, mirror: torch.Tensor):
        self._mirrors[param] = mirror

    @staticmethod
    def _kernel_eligible(p: torch.Tensor, state) -> bool:
        g = p.grad
        return (
            p.is_cuda
            and p.dtype == torch.float32
            and p.is_contiguous()
            and g.device == p.device
            and g.is_contiguous()
            and g.dtype in (torch.float32, torch.bfloat16)
            and all(
                s.device == p.device and s.dtype == torch.float32 and s.is_contiguous()
                for s in (state["exp_avg"], state["exp_avg_sq"])
            )
        )

    def _clip_coefficients(self, kernel_grads, fallback_grads):
        """device -> one-element fp32 tensor min(1, max_norm / (||g|| + 1e-6)),
        the norm taken over every grad of this step (clip_grad_norm_'s formula)."""
        sumsq = {}
        for device, grads in kernel_grads.items():
            sumsq[device] = torch.zeros(1, dtype=torch.float32, device=device)
            hip_ops().multi_grad_sumsq_(grads, sumsq[device])
        for device, g in fallback_grads:  # device: the param's, where its coefficient is needed
            if device not in sumsq:
                sumsq[device] = torch.zeros(1, dtype=torch.float32, device=device)
            sumsq[device].add_(g.float().square().sum().to(device))
        devices = list(sumsq)
        total = sumsq[devices[0]]
        for device in devices[1:]:  # params spread over devices: the copies order the streams
            total = total + sumsq[device].to(devices[0])
        clip = (self.max_grad_norm / (total.sqrt() + 1e-6)).clamp_(max=1.0)
        return {device: clip if device == devices[0] else clip.to(device) for device in devices}

    @torch.no_grad()
    def step(self, closure=None):
        loss = closure() if closure is not None else None
        lo, hi = self.clamp_trust_ratio
        buckets = {}  # (group index, step) -> ([p], [g], [m], [v], [kernel mirror], [(p, mirror, kernel mirror)])
        fallback = []  # (group, p, state)
        kernel_grads = {}  # device -> [g]
        for group_index, group in enumerate(self.param_groups):
            for p in group["params"]:
                if p.grad is None:
                    continue
                state = self.state[p]
                if len(state) == 0:
                    state["step"] = 0
                    state["exp_avg"] = torch.zeros_like(p, dtype=torch.float32)
                    state["exp_avg_sq"] = torch.zeros_like(p, dtype=torch.float32)
                state["step"] += 1
                if self._kernel_eligible(p, state):
                    mirror = self._mirrors.get(p)
                    kernel_mirror = mirror if (
                        mirror is not None and mirror.dtype == torch.bfloat16 and mirror.is_contiguous()
                        and mirror.device == p.device and mirror.numel() == p.numel()
                    ) else None
                    bucket = buckets.setdefault((group_index, state["step"]), ([], [], [], [], [], []))
                    bucket[0].append(p.data)
                    bucket[1].append(p.grad)
                    bucket[2].append(state["exp_avg"])
                    bucket[3].append(state["exp_avg_sq"])
                    bucket[4].append(kernel_mirror)
                    bucket[5].append((p, mirror, kernel_mirror))
                    kernel_grads.setdefault(p.device, []).append(p.grad)
                else:
                    fallback.append((group, p, state))

        clip = {}
        if self.max_grad_norm is not None and (buckets or fallback):
            clip = self._clip_coefficients(kernel_grads, [(p.device, p.grad) for _, p, _ in fallback])

        for (group_index, step_count), bucket in buckets.items():
            group = self.param_groups[group_index]
            beta1, beta2 = group["betas"]
            trust = hip_ops().multi_lamb_(
                bucket[0], bucket[1], bucket[2], bucket[3], bucket[4],
                group["lr"], beta1, beta2, group["eps"], group["weight_decay"], step_count,
                lo, hi, clip.get(bucket[0][0].device),
            )
            for (p, mirror, kernel_mirror), ratio in zip(bucket[5], trust.unbind(0)):
                self.last_trust_ratios[p] = ratio
                if mirror is not None and kernel_mirror is None:
                    mirror.copy_(p.data.to(mirror.dtype))

        for group, p, state in fallback:
            beta1, beta2 = group["betas"]
            g = p.grad.float().to(p.device)
            if p.device in clip:
                g = g * clip[p.device]  # a new tensor: p.grad itself stays as it is
            m, v = state["exp_avg"], state["exp_avg_sq"]
            m.mul_(beta1).add_(g, alpha=1 - beta1)
            v.mul_(beta2).addcmul_(g, g, value=1 - beta2)
            m_hat = m / (1 - beta1 ** state["step"])
            v_hat = v / (1 - beta2 ** state["step"])
            update = m_hat / (v_hat.sqrt() + group["eps"])
            if group["weight_decay"]:
                update = update + group["weight_decay"] * p.float()
            p_norm = p.detach().float().norm()
            u_norm = update.norm()
            trust_ratio = torch.where(
                (p_norm > 0) & (u_norm > 0), p_norm / u_norm, torch.ones_like(p_norm)
            ).clamp(lo, hi)
            p.data.sub_((update * (trust_ratio * group["lr"])).to(p.dtype))
            self.last_trust_ratios[p] = trust_ratio
            mirror = self._mirrors.get(p)
            if mirror is not None:
                mirror.copy_(p.data.to(mirror.dtype))
        return loss


class FusedAdamW(torch.optim.Optimizer):
    """AdamW whose step is one HIP kernel per parameter on the GPU.

    Master params must be fp32; an optional bf16 mirror (the live model param)
    is refreshed inside the same kernel -- this is the MI355X expression of the
    reference's "offloaded optimizer + parameter copy-back"
    (state_averager.py:515-536) with zero extra memory traffic.
    """

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01, mirrors=None):
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)
        super().__init__(params, defaults)
        self._mirrors = mirrors or {}

    def set_mirror(self, param: torch.Tensor, mirror: torch.Tensor):
        self._mirrors[param] = mirror

    @torch.no_grad()
    def step(self, closure=None):
        loss = closure() if closure is not None else None
        for group in self.param_groups:
            beta1, beta2 = group["betas"]
            # one multi-tensor launch per (step-count) bucket instead of one
            # kernel per parameter (round-1 profile: per-param launches were
            # a visible tail)
            mt_buckets = {}  # step -> ([p], [g], [m], [v], [mirror])
            for p in group["params"]:
                if p.grad is None:
                    continue
                state = self.state[p]
                if len(state) == 0:
                    state["step"] = 0
                    state["exp_avg"] = torch.zeros_like(p, dtype=torch.float32)
                    state["exp_avg_sq"] = torch.zeros_like(p, dtype=torch.float32)
                state["step"] += 1
                mirror = self._mirrors.get(p)
                if (
                    p.is_cuda
                    and p.dtype == torch.float32
                    and p.is_contiguous()
                    and p.grad.is_contiguous()
                    and p.grad.dtype in (torch.float32, torch.bfloat16)
                ):
                    kernel_mirror = mirror if (mirror is not None and mirror.dtype == torch.bfloat16
                                               and mirror.is_contiguous()) else None
                    bucket = mt_buckets.setdefault(state["step"], ([], [], [], [], [], []))
                    bucket[0].append(p.data)
                    bucket[1].append(p.grad)
                    bucket[2].append(state["exp_avg"])
                    bucket[3].append(state["exp_avg_sq"])
                    bucket[4].append(kernel_mirror)
                    bucket[5].append((p, mirror, kernel_mirror))
                elif p.is_cuda and p.dtype == torch.float32:
                    kernel_mirror = mirror if (mirror is not None and mirror.dtype == torch.bfloat16) else None
                    hip_ops().fused_adamw_(
                        p.data, p.grad.contiguous(), state["exp_avg"], state["exp_avg_sq"],
                        kernel_mirror, group["lr"], beta1, beta2, group["eps"], group["weight_decay"], state["step"],
                    )
                    if mirror is not None and kernel_mirror is None:
                        mirror.copy_(p.data.to(mirror.dtype))
                else:
                    g = p.grad.float()
                    state["exp_avg"].mul_(beta1).add_(g, alpha=1 - beta1)
                    state["exp_avg_sq"].mul_(beta2).addcmul_(g, g, value=1 - beta2)
                    bias_corr1 = 1 - beta1 ** state["step"]
                    bias_corr2 = 1 - beta2 ** state["step"]
                    denom = (state["exp_avg_sq"] / bias_corr2).sqrt_().add_(group["eps"])
                    update = state["exp_avg"] / bias_corr1 / denom + group["weight_decay"] * p.float()
                    p.data.add_(-group["lr"] * update.to(p.dtype))
                    if mirror is not None:
                        mirror.copy_(p.data.to(mirror.dtype))
            for step_count, bucket in mt_buckets.items():
                hip_ops().multi_adamw_(
                    bucket[0], bucket[1], bucket[2], bucket[3], bucket[4],
                    group["lr"], beta1, beta2, group["eps"], group["weight_decay"], step_count,
                )
                for p, mirror, kernel_mirror in bucket[5]:
                    if mirror is not None and kernel_mirror is None:
                        mirror.copy_(p.data.to(mirror.dtype))
        return loss
