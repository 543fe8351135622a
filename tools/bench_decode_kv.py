"""Decode step time and KV-cache size of a LLaMA-shaped model with the
fp16 and the MXFP8 KV cache (DecodeSession(kv_dtype=...)), as MHA and as
grouped-query attention with 4 kv heads.

Model and method of tools/bench_decode_gqa.py: build_llama(hidden=2048,
layers=8, heads=16, seq=2048, vocab=32000), kv_heads in {None (MHA), 4}.
Per batch size: one DecodeSession(capture=True, lm_head=True, smax=2048)
per (model, kv_dtype), each prefilled with the same 1792 random tokens so
the timed steps attend ~1.8k keys. Rounds alternate the variants in one
process; every round rewinds the session to position 1792, runs 20
warm-up steps, then times 200 steps (captured step plus lm head; step()
ends in a stream sync; only the greedy ids cross PCIe). Reported per
variant: median over rounds of the per-round median step time, min-max
over rounds, tokens/s, and the session's kv_cache_bytes.

    python tools/bench_decode_kv.py [--batches 8,64] [--rounds 3]
        [--variants mha-fp16,mha-mxfp8,gqa4-fp16,gqa4-mxfp8] [--steps 200]

--variants / --steps shorten a run for a kernel trace of one variant pair.
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HIDDEN, LAYERS, HEADS, SEQ, VOCAB = 2048, 8, 16, 2048, 32000
PROMPT, WARMUP, STEPS = 1792, 20, 200


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="8,64")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--variants",
                    default="mha-fp16,mha-mxfp8,gqa4-fp16,gqa4-mxfp8")
    ap.add_argument("--steps", type=int, default=STEPS)
    args = ap.parse_args()

    from trtlab_amd.engine.decode import DecodeSession
    from trtlab_amd.models import build_llama

    kvh_of = {"mha": None, "gqa4": 4}
    variants = [(v, *v.split("-")) for v in args.variants.split(",")]
    steps = args.steps
    graphs = {}
    for _, model, _ in variants:
        if model in graphs:
            continue
        t0 = time.time()
        graphs[model] = build_llama(batch=1, seq=SEQ, hidden=HIDDEN,
                                    layers=LAYERS, heads=HEADS, vocab=VOCAB,
                                    kv_heads=kvh_of[model])
        print(f"# built {model} graph in {time.time() - t0:.1f}s", flush=True)

    print(f"# llama hidden={HIDDEN} layers={LAYERS} heads={HEADS} "
          f"head_dim={HIDDEN // HEADS} smax={SEQ} prompt={PROMPT} "
          f"warmup={WARMUP} steps={steps} rounds={args.rounds}")
    for batch in [int(b) for b in args.batches.split(",")]:
        rng = np.random.RandomState(batch)
        prompt = rng.randint(1, VOCAB, (batch, PROMPT)).astype(np.int32)
        sess, kv_bytes = {}, {}
        for name, model, kv_dtype in variants:
            s = DecodeSession(graphs[model], batch=batch, smax=SEQ,
                              capture=True, lm_head=True, kv_dtype=kv_dtype)
            s.prefill(prompt)
            sess[name] = s
            kv_bytes[name] = s.kv_cache_bytes
            kc = s.layers[0]["kcache"]
            print(f"# b{batch} {name}: prefilled, kcache "
                  f"{tuple(kc.shape)} {kc.dtype}", flush=True)
        per_round = {name: [] for name, _, _ in variants}
        for r in range(args.rounds):
            for name, _, _ in variants:
                s = sess[name]
                s.set_pos(np.full(batch, PROMPT, np.int32))
                ids = np.full(batch, 7, np.int32)
                for _ in range(WARMUP):
                    ids = s.step(ids, return_ids=True).astype(np.int32)
                ts = np.empty(steps)
                for i in range(steps):
                    t0 = time.perf_counter()
                    ids = s.step(ids, return_ids=True).astype(np.int32)
                    ts[i] = time.perf_counter() - t0
                per_round[name].append(float(np.median(ts)) * 1e3)
                print(f"# b{batch} round {r} {name}: median "
                      f"{per_round[name][-1]:.4f} ms  mean "
                      f"{ts.mean() * 1e3:.4f} ms", flush=True)
        for name, _, _ in variants:
            v = np.array(per_round[name])
            med = float(np.median(v))
            print(f"batch={batch:<3d} {name:10s} step_ms median={med:.4f} "
                  f"min={v.min():.4f} max={v.max():.4f} "
                  f"tok/s={batch / med * 1e3:.0f} "
                  f"kv_cache_bytes={kv_bytes[name]} "
                  f"({kv_bytes[name] / 2**20:.0f} MiB)", flush=True)
        for s in sess.values():
            s.close()
        del sess


if __name__ == "__main__":
    main()
