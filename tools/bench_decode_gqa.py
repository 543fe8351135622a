"""Decode step time and KV-cache size of a LLaMA-shaped model as MHA and
as native grouped-query attention (kv_heads < heads).

Model: build_llama(hidden=2048, layers=8, heads=16, seq=2048,
vocab=32000), kv_heads in {None (MHA, the unchanged path), 4, 2}.
Per batch size: one DecodeSession(capture=True, lm_head=True, smax=2048)
per variant, each prefilled with the same 1792 random tokens so the timed
steps attend ~1.8k keys (the regime where the attention kernel, not the
launch count, carries the step). Rounds alternate the variants in one
process; every round rewinds the session to position 1792, runs 20
warm-up steps, then times 200 steps (step() ends in a stream sync; only
the greedy ids cross PCIe). Reported per variant: median over rounds of
the per-round median step time, min-max over rounds, tokens/s, and the
KV-cache bytes computed from the cache shapes.

    python tools/bench_decode_gqa.py [--batches 8,64] [--rounds 3]
                                     [--variants mha,gqa4,gqa2] [--steps 200]

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
    ap.add_argument("--variants", default="mha,gqa4,gqa2")
    ap.add_argument("--steps", type=int, default=STEPS)
    args = ap.parse_args()

    from trtlab_amd.engine.decode import DecodeSession
    from trtlab_amd.models import build_llama

    kvh_of = {"mha": None, "gqa4": 4, "gqa2": 2}
    variants = [(v, kvh_of[v]) for v in args.variants.split(",")]
    steps = args.steps
    graphs = {}
    for name, kvh in variants:
        t0 = time.time()
        graphs[name] = build_llama(batch=1, seq=SEQ, hidden=HIDDEN,
                                   layers=LAYERS, heads=HEADS, vocab=VOCAB,
                                   kv_heads=kvh)
        print(f"# built {name} graph in {time.time() - t0:.1f}s", flush=True)

    print(f"# llama hidden={HIDDEN} layers={LAYERS} heads={HEADS} "
          f"head_dim={HIDDEN // HEADS} smax={SEQ} prompt={PROMPT} "
          f"warmup={WARMUP} steps={steps} rounds={args.rounds}")
    for batch in [int(b) for b in args.batches.split(",")]:
        rng = np.random.RandomState(batch)
        prompt = rng.randint(1, VOCAB, (batch, PROMPT)).astype(np.int32)
        sess, kv_bytes = {}, {}
        for name, _ in variants:
            s = DecodeSession(graphs[name], batch=batch, smax=SEQ,
                              capture=True, lm_head=True)
            s.prefill(prompt)
            sess[name] = s
            kc = s.layers[0]["kcache"]
            kv_bytes[name] = 2 * s.n_layers * kc.numel() * kc.element_size()
            print(f"# b{batch} {name}: prefilled, kcache "
                  f"{tuple(kc.shape)}", flush=True)
        per_round = {name: [] for name, _ in variants}
        for r in range(args.rounds):
            for name, _ in variants:
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
        for name, _ in variants:
            v = np.array(per_round[name])
            med = float(np.median(v))
            print(f"batch={batch:<3d} {name:5s} step_ms median={med:.4f} "
                  f"min={v.min():.4f} max={v.max():.4f} "
                  f"tok/s={batch / med * 1e3:.0f} "
                  f"kv_cache_bytes={kv_bytes[name]} "
                  f"({kv_bytes[name] / 2**20:.0f} MiB)", flush=True)
        for s in sess.values():
            s.close()
        del sess


if __name__ == "__main__":
    main()
