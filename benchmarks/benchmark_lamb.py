#!/usr/bin/env python3
"""Optimizer-step A/B on the GPU: ops.FusedLamb(max_grad_norm=1.0) against
ClippingWrapper(ops.Lamb, 1.0) over the parameter-shape lists of ALBERT-base and
Llama-1B (fp32 masters, bf16 grads, random data).

Both optimizers live in one process and take their steps alternately, each step
between two stream events; the figure per optimizer is the median over --steps
steps after --warmup steps. The bytes-moved floor is what FusedLamb has to move
(BYTES_PER_ELEMENT below) over the HBM rate a streaming copy reaches on MI355X.

  python benchmarks/benchmark_lamb.py --models albert-base,llama-1b --steps 20
"""

import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

# bf16 grads, no mirror: norm pass reads g (2); stage 1 reads p, g, m, v (14) and
# writes m, v (8); stage 2 reads p, m, v (12) and writes p (4)
BYTES_PER_ELEMENT = 2 + 22 + 16
HBM_BYTES_PER_S = 6.3e12  # achievable streaming rate (8.0e12 is the spec peak)


def parameter_shapes(name):
    from hivemind_amd.models import AlbertConfig, AlbertForMaskedLM, LlamaConfig, LlamaForCausalLM

    config, cls = {
        "albert-base": (AlbertConfig.base(), AlbertForMaskedLM),
        "llama-1b": (LlamaConfig.llama_1b(), LlamaForCausalLM),
    }[name]
    with torch.device("meta"):
        model = cls(config)
    return [tuple(p.shape) for p in model.parameters()]


def make_optimizer(kind, shapes, seed, device):
    from hivemind_amd.moe.server.layers.optim import ClippingWrapper
    from hivemind_amd.ops import FusedLamb, Lamb, bind_grad

    gen = torch.Generator(device=device).manual_seed(seed)
    params = []
    for shape in shapes:
        p = torch.nn.Parameter(torch.randn(shape, device=device, generator=gen) * 0.02)
        bind_grad(p, torch.randn(shape, device=device, generator=gen).to(torch.bfloat16))
        params.append(p)
    if kind == "fused":
        return FusedLamb(params, lr=1e-3, weight_decay=0.01, max_grad_norm=1.0)
    return ClippingWrapper(Lamb(params, lr=1e-3, weight_decay=0.01), 1.0)


def bench_model(name, steps, warmup, device):
    shapes = parameter_shapes(name)
    elements = sum(torch.Size(s).numel() for s in shapes)
    # same seed: both start from the same parameters and gradients
    optimizers = {kind: make_optimizer(kind, shapes, 0, device) for kind in ("fused", "oracle")}
    times = {kind: [] for kind in optimizers}
    for step in range(warmup + steps):
        for kind, opt in optimizers.items():
            start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            opt.step()
            end.record()
            end.synchronize()
            if step >= warmup:
                times[kind].append(start.elapsed_time(end))
    fused_ms = statistics.median(times["fused"])
    oracle_ms = statistics.median(times["oracle"])
    floor_ms = BYTES_PER_ELEMENT * elements / HBM_BYTES_PER_S * 1e3
    return {
        "model": name,
        "tensors": len(shapes),
        "elements": elements,
        "fused_lamb_ms": round(fused_ms, 4),
        "fused_lamb_ms_min_max": [round(min(times["fused"]), 4), round(max(times["fused"]), 4)],
        "clipping_lamb_ms": round(oracle_ms, 4),
        "clipping_lamb_ms_min_max": [round(min(times["oracle"]), 4), round(max(times["oracle"]), 4)],
        "speedup": round(oracle_ms / fused_ms, 2),
        "bytes_floor_ms": round(floor_ms, 4),
        "fused_lamb_over_floor": round(fused_ms / floor_ms, 2),
    }


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--models", default="albert-base,llama-1b")
    parser.add_argument("--steps", type=int, default=20)
    parser.add_argument("--warmup", type=int, default=3)
    args = parser.parse_args()
    assert args.steps >= 20, "the median is taken over at least 20 steps"
    if not torch.cuda.is_available():
        raise SystemExit("benchmark_lamb.py measures on the GPU and found none")
    device = torch.device("cuda", 0)
    results = [bench_model(name, args.steps, args.warmup, device) for name in args.models.split(",")]
    print(json.dumps({
        "metric": "optimizer step time, median, stream events",
        "steps": args.steps,
        "warmup": args.warmup,
        "bytes_per_element": BYTES_PER_ELEMENT,
        "hbm_bytes_per_s": HBM_BYTES_PER_S,
        "device": torch.cuda.get_device_name(0),
        "results": results,
    }), flush=True)


if __name__ == "__main__":
    main()
