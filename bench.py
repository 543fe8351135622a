#!/usr/bin/env python3
"""trtlab_amd flagship benchmark: ResNet-50 fp16 batch=8 inference serving.

Measures the reference's headline metric (BASELINE.json: inferences/sec +
p99 latency, ResNet-50 fp16 b8) on N MI355X GPUs, one process per GPU
(data-parallel replicas, weights broadcast over RCCL at load). Synthetic
images, random-init calibrated weights (reference models/README.md:4-8).

Each step = one full serving iteration for one batch-8 request: H2D input
copy + graph-replayed fp16 forward + D2H output copy, pipelined across
multiple execution contexts (reference examples/00_TensorRT/inference.cc
pipeline). Weak scaling: per-GPU work is fixed as N grows.

Usage: python bench.py [--gpus N] [--steps K] [--warmup W]
                       [--dump-outputs DIR] [--full]
  (for N>1 the driver launches via torch.distributed.run, one rank per GPU)

A plain run sets up, warms up, times the K steps and prints the result
line. --dump-outputs DIR additionally writes the output bindings of the
last timed step as DIR/<binding>.npy (float32). --full adds the
single-inflight request-latency phase (config.p50_ms / config.p99_ms).
"""
from __future__ import annotations

import argparse
import json
import os
import time

import numpy as np

BASELINE_INF_S = 953.414  # reference examples/00_TensorRT/README.md:46 (V100)


class _TorchCommFallback:
    """torch.distributed stand-in matching the parallel.Communicator
    surface bench.py uses (barrier / all_reduce_scalar / broadcast via
    weights path / close). Only used if the owned RCCL layer fails on a
    multi-GPU node — see the warning at the construction site."""

    def __init__(self, rank, world, device):
        import torch
        import torch.distributed as dist

        self._torch, self._dist = torch, dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        torch.cuda.set_device(device)
        dist.init_process_group("nccl")
        self.rank, self.world, self.device = rank, world, device
        self._comm = self  # truthy: broadcast_weights takes the real path

    def barrier(self):
        self._dist.barrier()

    def all_reduce_scalar(self, v, op=None):
        t = self._torch.tensor([v], device="cuda",
                               dtype=self._torch.float64)
        self._dist.all_reduce(t, op=self._dist.ReduceOp.MAX)
        return float(t.item())

    def broadcast(self, ptr, nbytes, root=0, stream=0):
        import trtlab_amd

        C = trtlab_amd.native()
        staging = self._torch.empty(nbytes, dtype=self._torch.uint8,
                                    device="cuda")
        C.memory.memcpy_d2d(staging.data_ptr(), ptr, nbytes)
        self._torch.cuda.synchronize()
        self._dist.broadcast(staging, src=root)
        self._torch.cuda.synchronize()
        C.memory.memcpy_d2d(ptr, staging.data_ptr(), nbytes)

    def synchronize(self):
        self._torch.cuda.synchronize()

    def close(self):
        self._dist.destroy_process_group()


DUMP_BUDGET_BYTES = 48 << 20  # all dumped arrays together stay under 64 MB


def _binding_as_float(view: np.ndarray, dtype: str) -> np.ndarray:
    """Copy of an output binding as float32 (float64 for i32, exactly)."""
    if dtype == "bf16":  # bindings carry bf16 bit patterns
        bits = view.astype(np.uint16).astype(np.uint32) << 16
        return bits.view(np.float32)
    if dtype == "i32":
        return view.astype(np.float64)
    return view.astype(np.float32)


def dump_outputs(ctx, out_dir: str) -> None:
    """Write every output binding of `ctx` (as its caller would read them
    after synchronize) to out_dir/<binding>.npy. A binding too large for
    its share of the budget is reduced to a fixed seeded sample of its
    flattened elements, identical from run to run."""
    os.makedirs(out_dir, exist_ok=True)
    bindings = ctx.plan.outputs
    cap_bytes = DUMP_BUDGET_BYTES // max(len(bindings), 1)
    for b in bindings:
        arr = _binding_as_float(ctx.outputs[b["name"]], b["dtype"])
        cap = cap_bytes // arr.dtype.itemsize
        if arr.size > cap:
            idx = np.sort(np.random.RandomState(0).randint(0, arr.size, cap))
            arr = arr.reshape(-1)[idx]
        fname = "".join(ch if ch.isalnum() or ch in "-_." else "_"
                        for ch in b["name"])
        np.save(os.path.join(out_dir, fname + ".npy"), arr)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--contexts", type=int, default=3)
    ap.add_argument("--model", default="resnet50",
                    choices=["resnet50", "resnet101", "resnet152", "bert",
                             "bert-large", "gpt2", "llama", "vit"])
    ap.add_argument("--dtype", default="fp16",
                    choices=["fp16", "bf16", "int8", "fp8", "mxfp4", "mxfp8"])
    ap.add_argument("--no-autotune", action="store_true",
                    help="skip builder-time kernel tactic selection")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the last timed step's output bindings as "
                         "DIR/<binding>.npy (float32)")
    ap.add_argument("--full", action="store_true",
                    help="also run the single-inflight latency phase "
                         "(p50_ms / p99_ms)")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be >= 1")

    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", str(rank)))
    n_gpus = max(world, 1)

    import trtlab_amd
    from trtlab_amd.engine.planner import DT_F16, DT_I8, Planner
    from trtlab_amd.engine.runtime import NativeEngine
    from trtlab_amd.models import build_bert, build_resnet
    from trtlab_amd.parallel import Communicator, broadcast_weights

    # Device = local rank, wrapped by the visible device count so the
    # 2-rank single-GPU proof run works within a 1-GPU lease (identity
    # mapping on the driver's 8-GPU node).
    ndev = max(trtlab_amd.native().hip.device_count(), 1)
    local_rank = local_rank % ndev

    distributed = world > 1
    comm = None
    if distributed:
        # Owned RCCL communicator (csrc/runtime/comm.cpp): torchrun is only
        # the launcher — comm bring-up is our file-based uid rendezvous,
        # collectives run on our own streams (no torch.distributed).
        # Insurance: 1-GPU leases cannot exercise a real N>1 clique (RCCL
        # rejects co-located ranks), so if the owned path fails on the
        # multi-GPU node, fall back to torch.distributed with a LOUD
        # warning rather than losing the scaling measurement.
        try:
            comm = Communicator(rank=rank, world=world, device=local_rank)
        except Exception as e:  # noqa: BLE001
            import sys

            print(f"[bench] WARNING rank {rank}: owned RCCL comm failed "
                  f"({type(e).__name__}: {e}); falling back to "
                  f"torch.distributed", file=sys.stderr, flush=True)
            comm = _TorchCommFallback(rank, world, local_rank)

    # Build the plan (identical on every rank: same seed).
    if args.model == "bert":
        g = build_bert(batch=args.batch, seq=128, layers=12, seed=0)
        cfg_extra = {"seq_len": 128, "hidden": 768, "layers": 12}
    elif args.model == "bert-large":
        g = build_bert(batch=args.batch, seq=128, hidden=1024, heads=16,
                       layers=24, seed=0)
        cfg_extra = {"seq_len": 128, "hidden": 1024, "layers": 24}
    elif args.model == "gpt2":
        # full-sequence forward = prefill (causal online-softmax attention)
        from trtlab_amd.models import build_gpt2

        g = build_gpt2(batch=args.batch, seq=1024, layers=12, seed=0)
        cfg_extra = {"seq_len": 1024, "hidden": 768, "layers": 12,
                     "phase": "prefill"}
    elif args.model == "vit":
        # ViT-B/16: conv patch embed + 12-layer encoder (196 tokens)
        from trtlab_amd.models import build_vit

        g = build_vit(batch=args.batch, image=224, patch=16, seed=0)
        cfg_extra = {"image": 224, "patch": 16, "hidden": 768,
                     "layers": 12}
    elif args.model == "llama":
        # LLaMA-architecture prefill (RMSNorm + RoPE + SwiGLU, hd128)
        from trtlab_amd.models import build_llama

        g = build_llama(batch=args.batch, seq=512, hidden=2048, layers=8,
                        heads=16, seed=0)
        cfg_extra = {"seq_len": 512, "hidden": 2048, "layers": 8,
                     "phase": "prefill"}
    else:
        depth = int(args.model.replace("resnet", ""))
        g = build_resnet(depth, batch=args.batch, image=224, seed=0)
        cfg_extra = {"image": 224}
    from trtlab_amd.engine.planner import DT_BF16, DT_F8

    from trtlab_amd.engine.planner import DT_MX4, DT_MX8

    dtype = {"fp16": DT_F16, "bf16": DT_BF16, "int8": DT_I8,
             "fp8": DT_F8, "mxfp4": DT_MX4, "mxfp8": DT_MX8}[args.dtype]
    plan = Planner(dtype=dtype).compile(g)

    eng = NativeEngine(plan, device=local_rank,
                       autotune=not args.no_autotune)
    if distributed:
        # RCCL weight broadcast at load: rank 0's blob is
        # authoritative; replicas receive over xGMI (one fused in-place
        # broadcast of the whole blob on the engine's weight memory).
        broadcast_weights(eng, comm, src_rank=0)

    ctxs = [eng.create_context(capture=True) for _ in range(args.contexts)]

    rng = np.random.RandomState(123 + rank)
    if plan.inputs[0]["dtype"] == "i32":  # token-id models (llama)
        batch = rng.randint(1, 30000, plan.input_shape).astype(np.int32)
    else:
        batch = (rng.randn(*plan.input_shape) * 0.5).astype(np.float16)
    if args.dtype == "bf16":
        # bf16 bindings carry bit patterns (numpy has no bf16 dtype)
        from trtlab_amd.engine.planner import _bf16_bits

        batch = _bf16_bits(batch).reshape(plan.input_shape)
    for c in ctxs:
        np.copyto(c.input, batch)

    nc = len(ctxs)
    launch_t = [0.0] * nc
    lat_ms: list[float] = []

    def run_steps(k: int, record: bool):
        for i in range(k):
            c = ctxs[i % nc]
            if i >= nc:
                t_sync = time.perf_counter()
                c.synchronize()  # wait for this context's previous step
                if record:
                    lat_ms.append((time.perf_counter() - launch_t[i % nc]) * 1e3)
            launch_t[i % nc] = time.perf_counter()
            c.launch()
        for j, c in enumerate(ctxs):
            c.synchronize()
            if record:
                lat_ms.append((time.perf_counter() - launch_t[j]) * 1e3)

    # ---- warmup ----
    run_steps(args.warmup, record=False)

    # ---- timed region ----
    C = trtlab_amd.native()
    if distributed:
        comm.barrier()
    C.hip.device_synchronize()
    t0 = time.perf_counter()
    run_steps(args.steps, record=True)
    C.hip.device_synchronize()
    elapsed = time.perf_counter() - t0
    if distributed:
        # whole-job time = MAX over ranks (RCCL fp64 all-reduce)
        from trtlab_amd.parallel import OP_MAX

        elapsed = comm.all_reduce_scalar(elapsed, op=OP_MAX)
        comm.barrier()

    # ---- outputs of the last timed step (all contexts are synchronized;
    # the step ran on context (steps-1) % nc) ----
    if args.dump_outputs and rank == 0:
        dump_outputs(ctxs[(args.steps - 1) % nc], args.dump_outputs)

    # ---- --full: single-inflight latency phase (well-defined request
    # latency: H2D + graph replay + D2H, one at a time; not part of the
    # throughput measurement above) ----
    lat1 = []
    if args.full:
        for _ in range(64):
            t1 = time.perf_counter()
            ctxs[0].launch()
            ctxs[0].synchronize()
            lat1.append((time.perf_counter() - t1) * 1e3)
        if distributed:
            comm.barrier()

    if rank == 0:
        inf_s = n_gpus * args.steps * args.batch / elapsed
        ms_per_step = elapsed / args.steps * 1e3
        p99 = float(np.percentile(lat1, 99)) if lat1 else None
        p50 = float(np.percentile(lat1, 50)) if lat1 else None
        print(json.dumps({
            "metric": "inferences/sec",
            "value": round(inf_s, 2),
            "unit": "inf/s",
            "n_gpus": n_gpus,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(ms_per_step, 4),
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": round(inf_s / BASELINE_INF_S, 3),
            "dtype": args.dtype,
            "data": "synthetic",
            "config": {
                "model": args.model,
                "global_batch": args.batch * n_gpus,
                "batch_per_gpu": args.batch,
                **cfg_extra,
                "contexts": args.contexts,
                "parallelism": f"dp{n_gpus}",
                "p50_ms": p50,
                "p99_ms": p99,
                "latency_note": ("single-inflight request latency "
                                 "(H2D+forward+D2H, measured separately)"
                                 if args.full else
                                 "single-inflight latency not measured "
                                 "(run with --full)"),
                "pipelined_p99_ms": (float(np.percentile(lat_ms, 99))
                                     if lat_ms else None),
            },
        }), flush=True)

    if distributed:
        comm.barrier()
        comm.close()


if __name__ == "__main__":
    main()
