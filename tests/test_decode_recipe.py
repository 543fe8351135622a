"""The decode forward recipe needs no GPU: DecodeSession's recording
methods, borrowed by a stand-in that holds buffers with made-up addresses
and an `ops` object that launches nothing, must produce the golden step
and chunk launch traces (tests/golden/decode_launch_trace.json, recorded
on the GPU by tests/test_decode_trace_gpu.py --record).

This module also owns what both trace tests share: the two model shapes,
the recorder, the naming of pointers and the normal form of a trace.
"""
import json
import numbers
import os
import types

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                      "decode_launch_trace.json")

BATCH, SEQ, PROMPT, CHUNK = 2, 256, 5, 3
# inter: 4*hidden (GPT-2), round(hidden*8/3/64)*64 (build_llama's default)
MODELS = {
    "gpt2": dict(arch="gpt2", layers=2, hidden=128, heads=2, kv_heads=2,
                 hd=64, inter=512, vocab=512),
    "llama": dict(arch="llama", layers=2, hidden=256, heads=2, kv_heads=1,
                  hd=128, inter=704, vocab=512),
}
CACHES = {
    "dense_fp16": dict(paged=False, kv_dtype="fp16"),
    "paged_mxfp8": dict(paged=True, kv_dtype="mxfp8"),
}
# tensors a session holds under its own attribute names
SESSION_TENSORS = ("ids", "pos", "h", "x", "qkv", "att", "x2", "ff", "ff2",
                   "out", "logits", "gids", "h2", "tok", "posemb", "lnf_g",
                   "lnf_b")
_PTR = 1 << 32  # anything this large in an argument list is an address


class RecordingOps:
    """Appends [op name, positional args, keyword args] per call, then
    forwards to `ops` (None: launch nothing)."""

    def __init__(self, ops, log):
        self._ops, self._log = ops, log

    def __getattr__(self, name):
        fn = getattr(self._ops, name) if self._ops is not None else None

        def call(*args, **kw):
            self._log.append([name, list(args), dict(kw)])
            return fn(*args, **kw) if fn else None
        return call


def pointer_names(sess):
    """{data_ptr: name} of every tensor a session (or the stand-in) holds:
    its attributes, l{i}.{key}, pool.*, chunk{K}.{key}."""
    named = [(n, getattr(sess, n, None)) for n in SESSION_TENSORS]
    for i, lay in enumerate(sess.layers):
        named += [(f"l{i}.{k}", t) for k, t in lay.items()]
    pool = sess.kv_pool
    if pool is not None:
        named.append(("pool.table", pool.table))
        for short, lst in (("k", pool.kpools), ("v", pool.vpools),
                           ("ks", pool.kscales), ("vs", pool.vscales)):
            named += [(f"pool.{short}{i}", t)
                      for i, t in enumerate(lst or [])]
    for k, cb in sess._chunk_bufs_by_k.items():
        named += [(f"chunk{k}.{key}", t) for key, t in cb.items()]
    names = {}
    for name, t in named:
        if hasattr(t, "data_ptr"):
            assert names.setdefault(t.data_ptr(), name) == name
    return names


def normalize(log, names, prefill=False):
    """Normal form of a recorded pass. `stream` is dropped; `sync` is kept
    only where it is True; a keyword whose value is 0 is dropped (it equals
    the binding's default); a known address becomes its name, any other
    address `ptr<n>` by first appearance — or, in prefill, the one token
    "act" (prefill's private activation buffers may change roles)."""
    seen = {}

    def val(v):
        if isinstance(v, bool) or not isinstance(v, numbers.Integral):
            return v
        v = int(v)
        if v in names:
            return names[v]
        if v >= _PTR:
            return "act" if prefill else seen.setdefault(v, f"ptr{len(seen)}")
        return v

    out = []
    for op, args, kw in log:
        kw = dict(kw)
        kw.pop("stream")
        if kw.pop("sync"):
            kw["sync"] = True
        kw = {k: val(v) for k, v in kw.items()
              if isinstance(v, bool) or v != 0}
        out.append([op, [val(a) for a in args], kw])
    return out


def assert_no_sync(trace):
    for op, _, kw in trace:
        assert "sync" not in kw, f"{op} synchronises inside a pass"


def load_golden():
    with open(GOLDEN) as f:
        return json.load(f)


def as_json(trace):
    """What a trace looks like once it has been through the golden file."""
    return json.loads(json.dumps(trace))


# ------------------------------------------------------------ the stand-in
class _Buf:
    def __init__(self, ptr):
        self._ptr = ptr

    def data_ptr(self):
        return self._ptr


def _stand_in(model, cache, log):
    """An object with the attributes DecodeSession's recording methods
    read, over buffers that exist only as addresses."""
    from trtlab_amd.engine.decode import KV_DTYPES, DecodeSession
    from trtlab_amd.engine.planner import EPI_BIAS, EPI_BIAS_GELU, EPI_NONE

    class Recipe:
        _enqueue = DecodeSession._enqueue
        _enqueue_chunk = DecodeSession._enqueue_chunk
        _embed = DecodeSession._embed
        _head = DecodeSession._head
        _forward = DecodeSession._forward
        _kv = DecodeSession._kv

    m, c = MODELS[model], CACHES[cache]
    llama, mx = m["arch"] == "llama", c["kv_dtype"] == "mxfp8"
    count = iter(range(1, 1 << 20))

    def buf():
        return _Buf((1 << 40) + (next(count) << 12))

    s = Recipe()
    s._C = types.SimpleNamespace(ops=RecordingOps(None, log))
    s.stream = 0
    s.fused = False
    s.arch = m["arch"]
    s.batch, s.smax = BATCH, SEQ
    s.hidden, s.inter, s.vocab = m["hidden"], m["inter"], m["vocab"]
    s.heads, s.kv_heads, s.hd = m["heads"], m["kv_heads"], m["hd"]
    s.n_layers = m["layers"]
    s.qkv_w = (s.heads + 2 * s.kv_heads) * s.hd
    s._nkv = s.kv_heads if s.kv_heads != s.heads else 0
    s._kv_format = KV_DTYPES.index(c["kv_dtype"])
    s._scale = 1.0 / float(np.sqrt(float(s.hd)))
    s._epi_bias, s._epi_gelu, s._epi_none = EPI_BIAS, EPI_BIAS_GELU, EPI_NONE
    s.rms_eps, s.theta = 1e-5, 10000.0
    for name in SESSION_TENSORS:
        setattr(s, name, buf())
    if llama:
        s.lnf_b = None
        keys = ("rms1_g", "rms2_g", "qkv_w", "proj_w", "gate_w", "up_w",
                "down_w")
    else:
        s.ff2 = None
        keys = ("ln1_g", "ln1_b", "ln2_g", "ln2_b", "qkv_w", "qkv_b",
                "proj_w", "proj_b", "ff1_w", "ff1_b", "ff2_w", "ff2_b")
    dense = not c["paged"]
    s.layers = []
    for _ in range(s.n_layers):
        lay = {k: buf() for k in keys}
        lay["kcache"] = buf() if dense else None
        lay["vcache"] = buf() if dense else None
        lay["kscale"] = buf() if dense and mx else None
        lay["vscale"] = buf() if dense and mx else None
        s.layers.append(lay)
    s.kv_pool = None
    if c["paged"]:
        per_layer = range(s.n_layers)
        s.kv_pool = types.SimpleNamespace(
            table=buf(), max_pages=(SEQ + 63) // 64,
            kpools=[buf() for _ in per_layer],
            vpools=[buf() for _ in per_layer],
            kscales=[buf() for _ in per_layer] if mx else None,
            vscales=[buf() for _ in per_layer] if mx else None)
    cb = {k: buf() for k in ("ids", "h", "x", "x2", "qkv", "att", "ff",
                             "logits", "gids")}
    cb["K"] = CHUNK
    cb["ff2"] = buf() if llama else None
    s._chunk_bufs_by_k = {CHUNK: cb}
    return s


@pytest.mark.parametrize("cache", list(CACHES))
@pytest.mark.parametrize("model", list(MODELS))
def test_recipe_records_golden_step_and_chunk(model, cache):
    golden = load_golden()
    log = []
    s = _stand_in(model, cache, log)
    names = pointer_names(s)

    s._enqueue()
    step = normalize(log, names)
    assert_no_sync(step)
    assert as_json(step) == golden[f"{model}-{cache}-step"]

    del log[:]
    s._enqueue_chunk(s._chunk_bufs_by_k[CHUNK], BATCH, CHUNK)
    chunk = normalize(log, names)
    assert_no_sync(chunk)
    assert as_json(chunk) == golden[f"{model}-{cache}-chunk"]
