"""What a DecodeSession launches, compared with golden traces.

Two tiny models (GPT-2: 2 layers, hidden 128, 2 heads of 64; LLaMA: 2
layers, hidden 256, 2 heads of 128 over 1 kv head; vocab 512, smax 256,
batch 2, lm_head) each run as dense fp16 and as paged MXFP8. Per session
three passes are recorded: prefill of a 5-token prompt (padded to 128),
one step, verify_chunk with K = 3 — 12 traces. The recorder stands in for
`sess._C`: `hip` and `memory` pass through, every `ops` call is logged
and forwarded. test_decode_recipe.normalize gives the form compared:
step and chunk traces equal the goldens exactly, prefill traces equal
them with its private activation buffers masked to "act".

Inside a pass no launch may synchronise; prefill's closing lm-head GEMM,
after the pass, is the one launch with sync=True.

A keyword argument whose value is 0 is dropped before comparing, so that
passing a binding's default and leaving it out are the same launch. That
holds only where the default is 0; checked in csrc/ext.cpp for every
keyword these passes ever pass as 0:
    gemm_bt           bias, epi, tile
    rope              pos, chunk, kv_heads
    kv_append         pos, table, max_pages, kv_heads
    decode_attention  table, max_pages, kv_heads
    attention         kv_heads

The goldens (tests/golden/decode_launch_trace.json) are written by
    python tests/test_decode_trace_gpu.py --record
from whatever trtlab_amd/engine/decode.py is checked out.
"""
import functools
import json
import os
import sys

import numpy as np
import pytest

from test_decode_recipe import (BATCH, CACHES, CHUNK, GOLDEN, MODELS,
                                PROMPT, SEQ, RecordingOps, as_json,
                                assert_no_sync, load_golden, normalize,
                                pointer_names)

pytestmark = pytest.mark.gpu

PASSES = ("prefill", "step", "chunk")


class _RecordingC:
    def __init__(self, C, log):
        self.hip, self.memory = C.hip, C.memory
        self.ops = RecordingOps(C.ops, log)


def _graph(model):
    from trtlab_amd.models import build_gpt2, build_llama

    m = MODELS[model]
    kw = dict(batch=BATCH, seq=SEQ, hidden=m["hidden"], layers=m["layers"],
              heads=m["heads"], vocab=m["vocab"])
    if m["arch"] == "llama":
        return build_llama(kv_heads=m["kv_heads"], **kw)
    return build_gpt2(embeddings=True, **kw)


@functools.lru_cache(maxsize=None)
def record(model, cache):
    """{pass: normalised trace} of one session."""
    from trtlab_amd.engine.decode import DecodeSession

    sess = DecodeSession(_graph(model), batch=BATCH, smax=SEQ,
                         capture=False, lm_head=True, **CACHES[cache])
    log = []
    sess._C = _RecordingC(sess._C, log)
    rng = np.random.RandomState(3)
    vocab = MODELS[model]["vocab"]
    runs = (
        ("prefill", sess.prefill, rng.randint(1, vocab, (BATCH, PROMPT))),
        ("step", sess.step, rng.randint(1, vocab, BATCH)),
        ("chunk", sess.verify_chunk, rng.randint(1, vocab, (BATCH, CHUNK))),
    )
    traces = {}
    for name, run, tokens in runs:
        del log[:]
        assert np.isfinite(run(tokens.astype(np.int32))).all()
        traces[name] = normalize(log, pointer_names(sess),
                                 prefill=name == "prefill")
    sess.close()
    return traces


@pytest.mark.parametrize("which", PASSES)
@pytest.mark.parametrize("cache", list(CACHES))
@pytest.mark.parametrize("model", list(MODELS))
def test_launch_trace_matches_golden(model, cache, which):
    trace = record(model, cache)[which]
    # prefill's lm-head GEMM runs after the pass and is its only sync
    inside = trace[:-1] if which == "prefill" else trace
    assert_no_sync(inside)
    assert as_json(trace) == load_golden()[f"{model}-{cache}-{which}"]


def _write_golden():
    traces = {f"{m}-{c}-{p}": record(m, c)[p]
              for m in MODELS for c in CACHES for p in PASSES}
    body = ",\n".join(
        f' "{key}": [\n'
        + ",\n".join("  " + json.dumps(launch) for launch in trace)
        + "\n ]" for key, trace in traces.items())
    os.makedirs(os.path.dirname(GOLDEN), exist_ok=True)
    with open(GOLDEN, "w") as f:
        f.write("{\n" + body + "\n}\n")
    print(f"wrote {len(traces)} traces, "
          f"{sum(len(t) for t in traces.values())} launches, to {GOLDEN}")


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit("usage: python tests/test_decode_trace_gpu.py --record")
    sys.path.insert(0, os.path.dirname(os.path.dirname(
        os.path.abspath(__file__))))
    _write_golden()
