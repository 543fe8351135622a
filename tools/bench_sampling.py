"""Top-k / nucleus streams through GenerationEngine: host path against the
device path (device_truncation=True).

Model: build_llama(hidden=2048, layers=8, heads=16, vocab=32000), one
DecodeSession(capture=True, lm_head=True) per batch size, shared by both
engines. Every slot runs one stream with temperature=0.8, top_k=50,
top_p=0.9 and a one-token prompt; all streams are queued before the loop
starts, so with inline_step=True the engine runs them in lockstep and every
engine step emits `batch` tokens. Timed: wall time of the whole run divided
by engine steps (ms per emitted token-step), after an untimed 20-step run
of the same engine. Rounds alternate the two paths in one process; reported
per path: median over rounds, min-max.

  host    device_truncation=False: step() -> [B, vocab] fp32 logits D2H,
          GenerationEngine._sample per row (softmax + argsort in numpy)
  device  step(return_ids=True) + sample_tokens(temps, seeds, top_k, top_p)

    python tools/bench_sampling.py [--batches 8,64] [--rounds 3] [--steps 200]

--kernels N instead launches topk_topp_sample_rows and gumbel_argmax_rows
N times each on random [batch, 32000] logits: the workload for one
`rocprofv3 --kernel-trace --stats` run of the two kernels side by side.
"""
import argparse
import asyncio
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HIDDEN, LAYERS, HEADS, SMAX, VOCAB = 2048, 8, 16, 512, 32000
WARMUP = 20
PARAMS = dict(temperature=0.8, top_k=50, top_p=0.9)


async def _run(sess, device, batch, steps):
    from trtlab_amd.rpc.generation import GenerationEngine

    eng = GenerationEngine(sess, inline_step=True, device_truncation=device)
    subs = [asyncio.ensure_future(eng.submit([11 + b], steps, seed=b + 1,
                                             **PARAMS))
            for b in range(batch)]
    await asyncio.sleep(0)  # every stream queued before the first step
    t0 = time.perf_counter()
    eng.ensure_started()
    for sub in subs:
        _, q = await sub
        while await q.get() is not None:
            pass
    dt = time.perf_counter() - t0
    await eng.stop()
    assert eng.tokens_out == batch * steps, (eng.tokens_out, eng.steps)
    return dt / eng.steps * 1e3


def bench_engine(args):
    from trtlab_amd.engine.decode import DecodeSession
    from trtlab_amd.models import build_llama

    g = build_llama(batch=1, seq=SMAX, hidden=HIDDEN, layers=LAYERS,
                    heads=HEADS, vocab=VOCAB)
    print(f"# llama hidden={HIDDEN} layers={LAYERS} heads={HEADS} "
          f"vocab={VOCAB} smax={SMAX} warmup={WARMUP} steps={args.steps} "
          f"rounds={args.rounds} params={PARAMS}")
    for batch in [int(b) for b in args.batches.split(",")]:
        sess = DecodeSession(g, batch=batch, smax=SMAX, capture=True,
                             lm_head=True)
        per_round = {"host": [], "device": []}
        for r in range(args.rounds):
            for name in ("host", "device"):
                dev = name == "device"
                asyncio.run(_run(sess, dev, batch, WARMUP))
                ms = asyncio.run(_run(sess, dev, batch, args.steps))
                per_round[name].append(ms)
                print(f"# b{batch} round {r} {name}: {ms:.4f} ms/step",
                      flush=True)
        for name, v in per_round.items():
            v = np.array(v)
            med = float(np.median(v))
            print(f"batch={batch:<3d} {name:6s} ms_per_token_step "
                  f"median={med:.4f} min={v.min():.4f} max={v.max():.4f} "
                  f"tok/s={batch / med * 1e3:.0f}", flush=True)
        sess.close()


def run_kernels(args):
    import torch

    import trtlab_amd

    C = trtlab_amd.native()
    for batch in [int(b) for b in args.batches.split(",")]:
        x = torch.from_numpy((np.random.RandomState(batch).randn(
            batch, VOCAB) * 3).astype(np.float16)).cuda()
        out = torch.zeros(batch, dtype=torch.int32, device="cuda")
        t = torch.full((batch,), PARAMS["temperature"], device="cuda")
        k = torch.full((batch,), PARAMS["top_k"], dtype=torch.int32,
                       device="cuda")
        p = torch.full((batch,), PARAMS["top_p"], device="cuda")
        s = torch.arange(batch, dtype=torch.int32, device="cuda")
        for i in range(args.kernels):
            pos = torch.full((batch,), i, dtype=torch.int32, device="cuda")
            C.ops.topk_topp_sample_rows(
                x.data_ptr(), out.data_ptr(), temps=t.data_ptr(),
                top_k=k.data_ptr(), top_p=p.data_ptr(), seeds=s.data_ptr(),
                pos=pos.data_ptr(), M=batch, V=VOCAB)
            C.ops.gumbel_argmax_rows(
                x.data_ptr(), out.data_ptr(), temps=t.data_ptr(),
                seeds=s.data_ptr(), pos=pos.data_ptr(), M=batch, V=VOCAB)
        print(f"# b{batch}: {args.kernels} launches of each kernel")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="8,64")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--kernels", type=int, default=0)
    args = ap.parse_args()
    if args.kernels:
        run_kernels(args)
    else:
        bench_engine(args)


if __name__ == "__main__":
    main()
