#!/usr/bin/env python3
"""Flagship benchmark: ALBERT-base MLM training with hivemind_amd.Optimizer.

Measures the BASELINE.json headline metric -- samples/sec over the whole swarm
for collaborative ALBERT training (reference: examples/albert, ~20.9
samples/s/peer on 1080 Ti-class GPUs, target_batch_size 4096) -- on N MI355X
GPUs of one node, one process per GPU over RCCL/xGMI.

Usage:  python bench.py [--gpus N] [--steps K] [--warmup W] [--dump-outputs DIR] [--full]
For N>1 the driver launches this via torch.distributed.run with one rank per
GPU; ranks read RANK/LOCAL_RANK/WORLD_SIZE/MASTER_* from the environment.

A plain run sets up, warms up, times exactly K steps and prints one JSON result
line. --dump-outputs DIR additionally writes what the last timed step computed
(loss, logits, updated parameters) as DIR/<name>.npy so two builds can be
compared output for output. Everything beyond the headline figure belongs
behind --full.

Synthetic data (random token ids of the benchmark shape), random-init weights;
both are seeded, so the same arguments give the same inputs on every run.
"""

import argparse
import json
import math
import os
import sys
import time

import torch

BASELINE_SAMPLES_PER_SEC_PER_PEER = 20.9  # ALBERT collaborative trainer


def log(msg):
    print(f"[bench rank{os.environ.get('RANK', '0')}] {msg}", file=sys.stderr, flush=True)


DUMP_MAX_ELEMENTS = 4 * 1024 * 1024  # per dumped array: 16 MB as float32, 3 arrays < 64 MB


def _fixed_sample(flat, count, seed):
    """`count` elements of a 1-d tensor at fixed positions (seeded, sorted), or
    the whole tensor if it is no larger than that."""
    if flat.numel() <= count:
        return flat
    gen = torch.Generator(device="cpu").manual_seed(seed)
    index = torch.randint(0, flat.numel(), (count,), generator=gen).sort().values
    return flat[index.to(flat.device)]


def dump_outputs(dirname, loss, logits, parameters):
    """Write what the last timed step returned (loss, logits) and left behind
    (the updated model parameters) as float32 .npy files. Large arrays are
    reduced to a fixed seeded sample so the whole dump stays below 64 MB."""
    import numpy as np

    os.makedirs(dirname, exist_ok=True)
    parameters = list(parameters)
    per_param = max(1, DUMP_MAX_ELEMENTS // max(1, len(parameters)))
    arrays = {
        "loss": loss.detach().reshape(1),
        "logits": _fixed_sample(logits.detach().reshape(-1), DUMP_MAX_ELEMENTS, seed=0),
        "params": torch.cat([
            _fixed_sample(p.detach().reshape(-1), per_param, seed=1 + i).float()
            for i, p in enumerate(parameters)
        ]),
    }
    for name, tensor in arrays.items():
        np.save(os.path.join(dirname, f"{name}.npy"), tensor.float().cpu().numpy())
    log(f"wrote {', '.join(f'{name}.npy' for name in arrays)} to {dirname}")


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--gpus", type=int, default=1)
    parser.add_argument("--steps", type=int, default=24)
    parser.add_argument("--warmup", type=int, default=12)
    parser.add_argument("--batch", type=int, default=128, help="per-GPU samples per step")
    parser.add_argument("--seq-len", type=int, default=512)
    parser.add_argument("--target-batch-size", type=int, default=4096)
    parser.add_argument("--model", type=str, default="albert-base",
                        choices=["albert-base", "albert-large", "tiny", "llama-8b", "llama-1b", "llama-tiny"])
    parser.add_argument("--dpu", action="store_true",
                        help="delayed parameter updates: overlap averaging + optimizer step with compute")
    parser.add_argument("--powersgd-rank", type=int, default=0,
                        help="if > 0, average gradients with rank-r PowerSGD + error feedback (baseline config 3)")
    parser.add_argument("--grad-compression", type=str, default="bf16",
                        choices=["none", "bf16", "int8"],
                        help="gradient wire format on the RCCL/xGMI plane: bf16 cast (default) or "
                             "blockwise-int8 quantized butterfly (baseline config 2)")
    parser.add_argument("--hipgraph", type=str, default="auto", choices=["auto", "on", "off"],
                        help="capture the fwd+bwd region in a hipGraph and replay it per step "
                             "(auto: try, fall back to eager on capture failure)")
    parser.add_argument("--dump-outputs", type=str, default=None, metavar="DIR",
                        help="after the timed steps, write the last step's loss, logits and the updated "
                             "parameters as DIR/<name>.npy (float32; large arrays as a fixed seeded sample)")
    parser.add_argument("--full", action="store_true",
                        help="also run the measurements that the headline figure does not need; the "
                             "plain run already measures nothing else, so today this adds no work")
    args = parser.parse_args()

    world_size = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    n_gpus = world_size if world_size > 1 else args.gpus
    use_gpu = torch.cuda.is_available()

    # The metric is named "hivemind.Optimizer": its cost is the global step
    # (gradient averaging over xGMI + fused optimizer + epoch transition), so
    # the timed window must contain complete global steps at every N whatever
    # step count the driver chose (20x128 samples never
    # reached target_batch_size 4096 and the bench timed only fwd+bwd).
    # Epochs fire every ceil(target / (batch * N)) steps; raise the per-GPU
    # batch until >=2 epoch transitions fit in the timed window.
    min_batch = math.ceil(args.target_batch_size / max(1, n_gpus * max(args.steps // 2, 1)))
    if args.batch < min_batch:
        log(f"raising per-GPU batch {args.batch} -> {min_batch} so {args.steps} "
            f"timed steps at {n_gpus} GPUs span >=2 global steps (target {args.target_batch_size})")
        args.batch = min_batch

    import torch.distributed as dist

    bench_pg = None  # gloo subgroup for timing barriers: never touches the RCCL
    # communicators used by the (possibly background) averaging collectives
    if world_size > 1:
        backend = "nccl" if use_gpu else "gloo"
        dist.init_process_group(backend, rank=rank, world_size=world_size)
        bench_pg = dist.new_group(backend="gloo")
    if use_gpu:
        torch.cuda.set_device(local_rank)
        # TunableOp: pick the fastest hipBLASLt/rocBLAS algorithm per GEMM shape.
        # A pre-tuned table for the flagship config ships in profiles/ (measured
        # +10.5%: 93.3 -> 84.5 ms/step on ALBERT-base batch 128); any shapes not
        # in the table are tuned during the untimed warmup steps.
        try:
            import torch.cuda.tunable as tunable

            if os.environ.get("PYTORCH_TUNABLEOP_ENABLED", "1") == "0":
                raise RuntimeError("disabled via PYTORCH_TUNABLEOP_ENABLED=0")
            tunable.enable(True)
            tuned = os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                 "profiles", "tunableop_albert.csv")
            if not os.path.exists(tuned):
                tuned = os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                     "profiles", "tunableop_albert_b128.csv")
            if os.path.exists(tuned):
                try:
                    tunable.read_file(tuned)
                except Exception as e:
                    log(f"tunableop table not loaded: {e}")
            # tuning unknown shapes from scratch can add minutes of warmup
            # (observed: llama-1b blew a 200 s window); shapes missing from the
            # table just use hipBLASLt's default algorithm unless the caller
            # explicitly opts in to tuning
            tunable.tuning_enable(os.environ.get("PYTORCH_TUNABLEOP_TUNING", "0") == "1")
            if hasattr(tunable, "write_file_on_exit"):  # removed in torch 2.10
                tunable.write_file_on_exit(False)
        except Exception as e:
            log(f"TunableOp unavailable: {e}")
        device = torch.device("cuda", local_rank)
    else:
        device = torch.device("cpu")

    from hivemind_amd import DHT, Optimizer
    from hivemind_amd.models import AlbertConfig, AlbertForMaskedLM, LlamaConfig, LlamaForCausalLM
    from hivemind_amd.ops import FusedAdamW, hip_available

    if use_gpu and not hip_available():
        raise RuntimeError("HIP ops extension missing on a GPU node -- refusing to run a fallback bench")

    is_llama = args.model.startswith("llama")
    if args.model == "albert-base":
        config = AlbertConfig.base()
    elif args.model == "albert-large":
        config = AlbertConfig.large()
    elif args.model == "tiny":
        config = AlbertConfig.tiny()
    elif args.model == "llama-8b":
        config = LlamaConfig.llama_3_8b()
    elif args.model == "llama-1b":
        config = LlamaConfig.llama_1b()
    else:
        config = LlamaConfig.tiny()
    if not use_gpu:
        config.dtype = torch.float32  # CPU bf16 matmuls are pathologically slow
    max_pos = getattr(config, "max_position_embeddings", None)
    if max_pos is not None and args.seq_len > max_pos:
        log(f"clamping seq_len {args.seq_len} -> {max_pos} (model max positions)")
        args.seq_len = max_pos

    torch.manual_seed(1234 + rank)
    model_cls = LlamaForCausalLM if is_llama else AlbertForMaskedLM
    model = model_cls(config).to(device)
    log(f"model: {args.model}, {model.num_parameters()/1e6:.1f}M params, device={device}")

    # ---------------------------------------------------------------- swarm
    if world_size > 1:
        if rank == 0:
            dht = DHT(start=True)
            endpoint = [dht.endpoint]
        else:
            dht, endpoint = None, [None]
        dist.broadcast_object_list(endpoint, src=0)
        if rank != 0:
            dht = DHT(initial_peers=[endpoint[0]], start=True)
        dist.barrier()
    else:
        dht = DHT(start=True)

    opt = Optimizer(
        dht=dht,
        run_id="albert_bench",
        target_batch_size=args.target_batch_size,
        batch_size_per_step=args.batch,
        optimizer=lambda param_groups: FusedAdamW(param_groups, lr=2e-3, weight_decay=0.01),
        params=[{"params": list(model.parameters())}],
        offload_optimizer=True,
        matchmaking_time=1.0 if world_size > 1 else 0.5,
        averaging_timeout=120.0,
        reuse_grad_buffers=False,
        grad_rccl_wire_dtype=torch.bfloat16 if args.grad_compression == "bf16" else None,
        grad_rccl_compression="blockwise_int8" if args.grad_compression == "int8" else None,
        grad_averager_factory=(
            (lambda **kw: __import__("hivemind_amd.optim.power_sgd_averager", fromlist=["PowerSGDGradientAverager"])
             .PowerSGDGradientAverager(averager_rank=args.powersgd_rank, **kw))
            if args.powersgd_rank > 0 else None
        ),
        delay_optimizer_step=args.dpu,
        delay_grad_averaging=args.dpu,
        average_state_every=4,
        averager_opts=dict(
            request_timeout=0.5,
            min_group_size=min(2, n_gpus),
            target_group_size=n_gpus if n_gpus > 1 else None,
        ),
        tracker_opts=dict(min_refresh_period=0.2, default_refresh_period=0.5, max_refresh_period=2.0),
        verbose=rank == 0,
    )

    def make_batch():
        input_ids = torch.randint(0, config.vocab_size, (args.batch, args.seq_len), device=device)
        labels = input_ids.clone()
        if not is_llama:
            # mask 15% of positions for MLM, rest ignored in the loss
            mask = torch.rand(labels.shape, device=device) > 0.15
            labels[mask] = -100
        return input_ids, labels

    graph_state = {}
    # the logits outlive their step only when they are to be dumped (rank 0 writes)
    keep_logits = args.dump_outputs is not None and rank == 0

    def try_capture_hipgraph():
        """Capture fwd+bwd once; per-step we copy fresh data into the static
        buffers and replay (the north star's "capture launch-bound inner
        loops in hipGraphs"). The optimizer/averaging logic stays eager."""
        static_ids, static_labels = make_batch()
        # canonical capture recipe: warm up on a SIDE stream so AccumulateGrad
        # nodes bind to a non-default stream (a default-stream warmup made the
        # later capture core-dump on ROCm), then drop the autograd graph refs
        side = torch.cuda.Stream(device)
        side.wait_stream(torch.cuda.current_stream(device))
        with torch.cuda.stream(side):
            for _ in range(2):
                loss, _ = model(static_ids, labels=static_labels)
                loss.backward()
        torch.cuda.current_stream(device).wait_stream(side)
        del loss
        opt.zero_grad(set_to_none=False)
        torch.cuda.synchronize(device)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            static_loss, static_logits = model(static_ids, labels=static_labels)
            static_loss.backward()
        graph_state.update(graph=graph, ids=static_ids, labels=static_labels, loss=static_loss)
        if keep_logits:
            # holding the captured logits keeps their block out of the graph
            # pool's reuse, so each replay leaves them intact for the dump
            graph_state.update(logits=static_logits)
        del static_logits
        log("hipGraph capture of fwd+bwd succeeded")

    def one_step():
        if graph_state:
            input_ids, labels = make_batch()
            graph_state["ids"].copy_(input_ids)
            graph_state["labels"].copy_(labels)
            graph_state["graph"].replay()
            loss = graph_state["loss"]
            opt.step()
            opt.zero_grad(set_to_none=False)  # keep the graph's grad buffers
            return loss, graph_state.get("logits")
        input_ids, labels = make_batch()
        loss, logits = model(input_ids, labels=labels)
        loss.backward()
        opt.step()
        opt.zero_grad()
        return loss, (logits if keep_logits else None)

    if use_gpu and args.hipgraph in ("auto", "on"):
        try:
            try_capture_hipgraph()
        except Exception as e:
            if args.hipgraph == "on":
                raise
            log(f"hipGraph capture failed ({e!r}); running eager")
            graph_state.clear()
            opt.zero_grad()

    def sync():
        if use_gpu:
            torch.cuda.synchronize(device)
        if world_size > 1:
            dist.barrier(group=bench_pg)

    if world_size > 1:
        # pre-warm the full-world communicator the averaging rounds will use
        # (cached member-only group): a communicator problem then fails at
        # startup instead of hanging the first global step
        from hivemind_amd.averaging.rccl import get_process_group_for_ranks

        warm_pg = get_process_group_for_ranks(list(range(world_size)))
        warm = torch.ones(1, device=device if use_gpu else "cpu")
        dist.all_reduce(warm, group=warm_pg)
        log(f"averaging communicator warm: {warm.item():.0f} == {world_size}")

        # measure the steady swarm, not the discovery transient: wait until the
        # progress tracker on every rank sees the whole world before warmup
        deadline = time.perf_counter() + 30.0
        while opt.tracker.global_progress.num_peers < world_size and time.perf_counter() < deadline:
            time.sleep(0.1)
        log(f"tracker sees {opt.tracker.global_progress.num_peers}/{world_size} peers")
        sync()

    log(f"warmup: {args.warmup} steps")
    for i in range(args.warmup):
        one_step()
    sync()

    log(f"timing: {args.steps} steps")
    epoch_before = opt.local_epoch
    step_times = []
    epoch_steps = []  # wall time of steps in which an epoch transition landed
    last_outputs = None
    t0 = time.perf_counter()
    for i in range(args.steps):
        e0, s0 = opt.local_epoch, time.perf_counter()
        if keep_logits and i == args.steps - 1:
            last_outputs = one_step()
        else:
            one_step()
        dt = time.perf_counter() - s0
        step_times.append(dt)
        if opt.local_epoch != e0:
            epoch_steps.append(dt)
    sync()
    elapsed = time.perf_counter() - t0
    epochs_completed = opt.local_epoch - epoch_before

    # every rank must have amortized >=1 full global step, else the headline
    # metric was not measured -- fail loudly rather than report fwd+bwd only
    if epochs_completed < 1:
        log(f"FATAL: timed window contained {epochs_completed} epoch transitions; "
            f"the metric requires >=1 full global step (averaging + optimizer)")
        raise RuntimeError("bench timed window contained no global step")

    # take the max elapsed across ranks (slowest peer defines the swarm rate);
    # runs on the gloo subgroup so it cannot interleave with RCCL averaging
    if world_size > 1:
        t = torch.tensor([elapsed], dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX, group=bench_pg)
        elapsed = float(t.item())

    if last_outputs is not None:
        if args.dpu:
            # a delayed update may still be writing the parameters
            opt.state_averager.step(wait_for_delayed_updates=True)
        dump_outputs(args.dump_outputs, *last_outputs, model.parameters())

    total_samples = args.steps * args.batch * n_gpus
    samples_per_sec = total_samples / elapsed
    ms_per_step = elapsed / args.steps * 1000.0

    if rank == 0:
        result = {
            "metric": ("samples/sec (whole swarm) ALBERT-base hivemind.Optimizer" if not is_llama
                       else f"samples/sec (whole swarm) {args.model} hivemind.Optimizer"
                       + (" + DPU" if args.dpu else "")),
            "value": round(samples_per_sec, 2),
            "unit": "samples/s",
            "n_gpus": n_gpus,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(ms_per_step, 2),
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": round(samples_per_sec / (BASELINE_SAMPLES_PER_SEC_PER_PEER * n_gpus), 2),
            "dtype": "bf16" if use_gpu else "fp32",
            "data": "synthetic",
            "epochs_in_timed_window": epochs_completed,
            "grad_data_plane": (opt.grad_averager.last_data_plane if opt.grad_averager is not None else None),
            # per-step walls are enqueue-side (GPU work is async; epoch steps
            # absorb pipeline backlog at their sync points) -- the headline
            # ms_per_step is measured between device-synchronized barriers
            "per_step_timing": "async-enqueue",
            "global_step_ms": round(1000.0 * sum(epoch_steps) / len(epoch_steps), 2) if epoch_steps else None,
            "plain_step_ms": round(
                1000.0 * (sum(step_times) - sum(epoch_steps)) / max(1, len(step_times) - len(epoch_steps)), 2
            ),
            "config": {
                "model": args.model,
                "dpu": args.dpu,
                "powersgd_rank": args.powersgd_rank or None,
                "grad_compression": args.grad_compression,
                "global_batch": args.target_batch_size,
                "per_gpu_batch": args.batch,
                "seq_len": args.seq_len,
                "parallelism": f"dp{n_gpus}",
            },
        }
        print(json.dumps(result), flush=True)

    opt.shutdown()
    dht.shutdown()
    if world_size > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    try:
        main()
    except BaseException:
        import traceback

        traceback.print_exc()
        # daemon threads (DHT loop, tracker) must not keep a failed bench alive
        os._exit(1)
    # Exit normally so profilers (rocprofv3) can finalize their databases in
    # C-level destructors, but arm a watchdog in case a lingering non-daemon
    # thread would otherwise hang the process after a successful run.
    import threading

    watchdog = threading.Timer(30.0, lambda: os._exit(0))
    watchdog.daemon = True
    watchdog.start()
    sys.exit(0)
