"""Native grouped-query attention end to end on the GPU: the captured
engine and LLaMA DecodeSessions (dense, paged, prefill, chunked
verification, speculative decoding) on kv_heads < heads graphs.
Tolerances are the ones tests/test_engine_gpu.py uses for the same
comparisons on MHA graphs."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

B, T = 2, 6


def _rel(a, b):
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-6))


def test_gqa_engine_matches_reference():
    from trtlab_amd.engine.planner import Planner
    from trtlab_amd.engine.reference import run_reference
    from trtlab_amd.engine.runtime import NativeEngine
    from trtlab_amd.models import build_llama

    g = build_llama(batch=2, seq=128, hidden=512, heads=4, kv_heads=2,
                    layers=2)
    plan = Planner().compile(g)
    ctx = NativeEngine(plan).create_context(capture=True)
    ids = np.random.RandomState(5).randint(
        1, 30000, size=plan.input_shape).astype(np.int32)
    out = ctx.infer(ids).astype(np.float32)
    ref = run_reference(plan, ids)
    assert np.isfinite(out).all()
    assert _rel(out, ref) < 0.08, _rel(out, ref)


@pytest.fixture(scope="module", params=[1, 2])
def model(request):
    """(graph, kv heads, tokens, per-position reference), shared by the
    session tests of one kv-head count."""
    from trtlab_amd.engine.planner import Planner
    from trtlab_amd.engine.reference import run_reference
    from trtlab_amd.models import build_llama

    k = request.param
    g = build_llama(batch=B, seq=T, hidden=512, heads=4, kv_heads=k,
                    layers=2, vocab=5000)
    toks = np.random.RandomState(9).randint(1, 5000, (B, T)).astype(np.int32)
    ref = run_reference(Planner().compile(g), toks.reshape(-1))
    return g, k, toks, ref.reshape(B, T, -1)


@pytest.mark.parametrize("paged", [False, True])
def test_gqa_sessions_track_reference(model, paged):
    from trtlab_amd.engine.decode import DecodeSession

    g, k, toks, ref_all = model
    s = DecodeSession(g, batch=B, capture=False, paged=paged)
    assert s.arch == "llama" and s.hd == 128
    assert s.heads == 4 and s.kv_heads == k
    for i in range(T):
        out = s.step(toks[:, i])
        err = _rel(out, ref_all[:, i])
        assert err < 0.05, (paged, i, err)
    s.close()


def test_gqa_captured_matches_eager(model):
    from trtlab_amd.engine.decode import DecodeSession

    g, _, toks, _ = model
    s = DecodeSession(g, batch=B, capture=True)
    e = DecodeSession(g, batch=B, capture=False)
    for i in range(4):
        a, b = s.step(toks[:, i]), e.step(toks[:, i])
    assert np.allclose(a, b, atol=1e-3)
    s.close()
    e.close()


def test_gqa_verify_chunk_matches_steps(model):
    from trtlab_amd.engine.decode import DecodeSession

    g, _, toks, _ = model
    s = DecodeSession(g, batch=B, capture=False, lm_head=True)
    first = s.verify_chunk(toks[:, :1])
    s.add_pos(np.ones(B, np.int64))
    rest = s.verify_chunk(toks[:, 1:])
    seq = DecodeSession(g, batch=B, capture=False, lm_head=True)
    for i in range(T):
        lg = seq.step(toks[:, i])
        got = first[:, 0] if i == 0 else rest[:, i - 1]
        np.testing.assert_allclose(got, lg, rtol=3e-2, atol=3e-2)
    s.close()
    seq.close()


def test_gqa_cache_shapes_and_pool_check(model):
    from trtlab_amd.engine.decode import DecodeSession, PagedKVPool

    g, k, _, _ = model
    s = DecodeSession(g, batch=B, capture=False)
    smax = s.smax
    assert tuple(s.layers[0]["kcache"].shape) == (B, k, smax, 128)
    assert tuple(s.layers[0]["vcache"].shape) == (B, k, smax, 128)
    assert tuple(s.qkv.shape) == (B, (4 + 2 * k) * 128)
    s.close()
    p = DecodeSession(g, batch=B, capture=False, paged=True)
    pages = B * ((p.smax + 63) // 64)
    assert tuple(p.kv_pool.kpools[0].shape) == (pages, 64, k, 128)
    assert p.layers[0]["kcache"] is None
    p.close()
    pool = PagedKVPool(2, 4, B, num_pages=4, max_pages_per_slot=2,
                       head_dim=128)  # sized for query heads: too wide
    with pytest.raises(ValueError):
        DecodeSession(g, batch=B, capture=False, paged=pool)
    ok = PagedKVPool(2, k, B, num_pages=4, max_pages_per_slot=2,
                     head_dim=128)
    DecodeSession(g, batch=B, capture=False, paged=ok).close()


def test_gqa_fused_rejected(model):
    from trtlab_amd.engine.decode import DecodeSession

    with pytest.raises(ValueError):
        DecodeSession(model[0], batch=B, lm_head=True, fused=True)


@pytest.mark.parametrize("paged", [False, True])
def test_gqa_prefill_matches_sequential(paged):
    from trtlab_amd.engine.decode import DecodeSession
    from trtlab_amd.models import build_llama

    g = build_llama(batch=2, seq=256, hidden=512, heads=4, kv_heads=2,
                    layers=2, vocab=5000)
    rng = np.random.RandomState(13)
    prompt = rng.randint(1, 5000, (2, 100)).astype(np.int32)
    nxt = rng.randint(1, 5000, (2, 3)).astype(np.int32)
    a = DecodeSession(g, batch=2, smax=256, capture=False, paged=paged)
    for t in range(100):
        out_seq = a.step(prompt[:, t])
    b = DecodeSession(g, batch=2, smax=256, capture=False, paged=paged)
    out_pre = b.prefill(prompt)
    assert _rel(out_pre, out_seq) < 0.05
    for t in range(3):
        sa, sb = a.step(nxt[:, t]), b.step(nxt[:, t])
        assert _rel(sb, sa) < 0.05, t
    a.close()
    b.close()


def test_gqa_speculative_decoding_invariant():
    """GQA target, mismatched 1-layer MHA draft: the emitted tokens are
    the target's own greedy tokens."""
    from trtlab_amd.engine.decode import DecodeSession, SpeculativeDecoder
    from trtlab_amd.models import build_llama

    g = build_llama(batch=2, seq=96, hidden=512, layers=2, heads=4,
                    kv_heads=2, seed=0, vocab=2000)
    g_diff = build_llama(batch=2, seq=96, hidden=512, layers=1, heads=4,
                         seed=5, vocab=2000)
    seed_tok = np.array([17, 23], np.int32)
    steps = 10
    base = DecodeSession(g, batch=2, smax=96, capture=False, lm_head=True)
    cur, ref = seed_tok, []
    for _ in range(steps):
        cur = base.step(cur).argmax(-1).astype(np.int32)
        ref.append(cur)
    base.close()
    t = DecodeSession(g, batch=2, smax=96, capture=False, lm_head=True)
    d = DecodeSession(g_diff, batch=2, smax=96, capture=False, lm_head=True)
    toks, _ = SpeculativeDecoder(t, d, k=3).generate(seed_tok, steps)
    np.testing.assert_array_equal(toks, np.stack(ref, axis=1))
    t.close()
    d.close()
