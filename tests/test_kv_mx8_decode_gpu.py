"""MXFP8 KV cache end to end on the GPU: LLaMA DecodeSessions with
kv_dtype="mxfp8" (dense, paged, prefill, chunked verification,
speculative decoding) on the models of tests/test_gqa_decode_gpu.py
(hidden 512, 4 heads of 128, kv_heads in {1, 2, 4}, 2 layers).

Three kinds of check:
  * reference tracking: per position against
    run_reference(kv_format="mxfp8"), the CPU definition (every K/V head
    row through the host MX codec). The bound is the project's bound for
    session-vs-reference, _rel < 0.05; the measured values are printed
    next to the fp16 session's against the plain reference (NOTES.md,
    "MXFP8 KV cache", records both).
  * exact plumbing: layer 0's K/V do not depend on attention, so the
    mxfp8 session's layer-0 codes and scale bytes must equal
    quantize_mxfp8 of the fp16 session's layer-0 cache rows bit for bit.
    Both sessions run the same GEMM kernels on the same inputs in one
    process: the raw-op GEMMs pick their tile from the shape alone
    (tile=0 heuristic, no timing), so no tactic needs pinning.
  * the criteria tests/test_gqa_decode_gpu.py uses for captured vs
    eager, verify_chunk vs steps and speculative decoding, unchanged.
"""
import numpy as np
import pytest

from trtlab_amd.engine.mx import quantize_mxfp8

pytestmark = pytest.mark.gpu

B, T = 2, 6
HD = 128


def _rel(a, b):
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-6))


def _llama(kv, **kw):
    from trtlab_amd.models import build_llama

    args = dict(batch=B, seq=T, hidden=512, heads=4, layers=2, vocab=5000,
                kv_heads=None if kv == 4 else kv)
    args.update(kw)
    return build_llama(**args)


@pytest.fixture(scope="module", params=[1, 2, 4])
def model(request):
    """(graph, kv heads, tokens, mxfp8 reference, plain reference) per
    position, shared by the session tests of one kv-head count."""
    from trtlab_amd.engine.planner import Planner
    from trtlab_amd.engine.reference import run_reference

    k = request.param
    g = _llama(k)
    toks = np.random.RandomState(9).randint(1, 5000, (B, T)).astype(np.int32)
    plan = Planner().compile(g)
    ref_mx = run_reference(plan, toks.reshape(-1), kv_format="mxfp8")
    ref = run_reference(plan, toks.reshape(-1))
    return g, k, toks, ref_mx.reshape(B, T, -1), ref.reshape(B, T, -1)


def _session(g, **kw):
    from trtlab_amd.engine.decode import DecodeSession

    kw.setdefault("batch", B)
    kw.setdefault("capture", False)
    return DecodeSession(g, **kw)


@pytest.mark.parametrize("paged", [False, True])
def test_mx8_sessions_track_reference(model, paged):
    g, k, toks, ref_mx, ref = model
    s = _session(g, paged=paged, kv_dtype="mxfp8")
    f = _session(g, paged=paged)
    assert s.kv_dtype == "mxfp8" and f.kv_dtype == "fp16"
    assert s.arch == "llama" and s.hd == HD and s.kv_heads == k
    errs, errs16 = [], []
    for i in range(T):
        errs.append(_rel(s.step(toks[:, i]), ref_mx[:, i]))
        errs16.append(_rel(f.step(toks[:, i]), ref[:, i]))
    print(f"kv_heads={k} paged={paged}: mxfp8 session vs mxfp8 reference "
          f"_rel per position {['%.4f' % e for e in errs]} max "
          f"{max(errs):.4f}; fp16 session vs reference "
          f"{['%.4f' % e for e in errs16]} max {max(errs16):.4f}")
    s.close()
    f.close()
    assert max(errs) < 0.05, (paged, errs)


def _layer0_rows(s, name, positions):
    """Layer 0's cache rows [B, kv_heads, len(positions), W] of buffer
    `name` ("k", "v" caches; "kscale", "vscale"), dense or through the
    host page table."""
    if s.kv_pool is None:
        key = {"k": "kcache", "v": "vcache"}.get(name, name)
        return s.layers[0][key][:, :, positions].cpu().numpy()
    pool = s.kv_pool
    src = {"k": pool.kpools, "v": pool.vpools, "kscale": pool.kscales,
           "vscale": pool.vscales}[name][0].cpu().numpy()
    out = []
    for b in range(s.batch):
        rows = []
        for t in positions:
            page = int(pool._table_host[b, t >> 6])
            assert page >= 0
            rows.append(src[page, t & 63])  # [kv_heads, W]
        out.append(np.stack(rows, 1))
    return np.stack(out)


def _assert_layer0_quantised(mx, fp, positions):
    for name in ("k", "v"):
        rows = _layer0_rows(fp, name, positions).astype(np.float32)
        assert np.abs(rows).max() > 0
        # the host codec and the device differ on an all-zero block only
        assert not (rows.reshape(-1, 32) == 0).all(1).any()
        codes, scales = quantize_mxfp8(rows.reshape(-1, HD))
        got_c = _layer0_rows(mx, name, positions)
        got_s = _layer0_rows(mx, name + "scale", positions)
        assert got_c.dtype == np.uint8 and got_s.dtype == np.uint8
        assert np.array_equal(got_c.reshape(-1, HD), codes), name
        assert np.array_equal(got_s.reshape(-1, HD // 32), scales), name


@pytest.mark.parametrize("paged", [False, True])
def test_mx8_layer0_cache_is_quantised_fp16_cache(model, paged):
    g, _, toks, _, _ = model
    mx = _session(g, paged=paged, kv_dtype="mxfp8")
    fp = _session(g, paged=paged)
    for i in range(4):
        mx.step(toks[:, i])
        fp.step(toks[:, i])
    _assert_layer0_quantised(mx, fp, list(range(4)))
    mx.close()
    fp.close()


@pytest.mark.parametrize("paged", [False, True])
def test_mx8_prefill(paged):
    """prefill reads the unquantised qkv, so its return matches the fp16
    session's (captured-vs-eager criterion); the range append quantises
    into the cache: layer-0 rows below the prompt length are the
    quantised fp16 rows. The steps after it attend the quantised cache
    and stay finite."""
    g = _llama(2, seq=256)
    rng = np.random.RandomState(13)
    prompt = rng.randint(1, 5000, (B, 100)).astype(np.int32)
    mx = _session(g, smax=256, paged=paged, kv_dtype="mxfp8")
    fp = _session(g, smax=256, paged=paged)
    a, b = mx.prefill(prompt), fp.prefill(prompt)
    print(f"prefill return mxfp8 vs fp16: max abs {np.abs(a - b).max():.3g}")
    assert np.allclose(a, b, atol=1e-3)
    _assert_layer0_quantised(mx, fp, list(range(100)))
    nxt = rng.randint(1, 5000, B).astype(np.int32)
    sa, sb = mx.step(nxt), fp.step(nxt)
    print(f"step after prefill mxfp8 vs fp16: _rel {_rel(sa, sb):.4f}")
    assert np.isfinite(sa).all()
    mx.close()
    fp.close()


def test_mx8_captured_matches_eager(model):
    g, _, toks, _, _ = model
    s = _session(g, capture=True, kv_dtype="mxfp8")
    e = _session(g, capture=False, kv_dtype="mxfp8")
    for i in range(4):
        a, b = s.step(toks[:, i]), e.step(toks[:, i])
    assert np.allclose(a, b, atol=1e-3)
    s.close()
    e.close()


def test_mx8_verify_chunk_matches_steps(model):
    g, _, toks, _, _ = model
    s = _session(g, lm_head=True, kv_dtype="mxfp8")
    first = s.verify_chunk(toks[:, :1])
    s.add_pos(np.ones(B, np.int64))
    rest = s.verify_chunk(toks[:, 1:])
    seq = _session(g, lm_head=True, kv_dtype="mxfp8")
    for i in range(T):
        lg = seq.step(toks[:, i])
        got = first[:, 0] if i == 0 else rest[:, i - 1]
        np.testing.assert_allclose(got, lg, rtol=3e-2, atol=3e-2)
    s.close()
    seq.close()


def test_mx8_speculative_decoding_invariant():
    """mxfp8 GQA target, mismatched 1-layer fp16 draft: the emitted
    tokens are the mxfp8 target's own greedy tokens."""
    from trtlab_amd.engine.decode import SpeculativeDecoder
    from trtlab_amd.models import build_llama

    g = build_llama(batch=2, seq=96, hidden=512, layers=2, heads=4,
                    kv_heads=2, seed=0, vocab=2000)
    g_diff = build_llama(batch=2, seq=96, hidden=512, layers=1, heads=4,
                         seed=5, vocab=2000)
    seed_tok = np.array([17, 23], np.int32)
    steps = 10
    base = _session(g, smax=96, lm_head=True, kv_dtype="mxfp8")
    cur, ref = seed_tok, []
    for _ in range(steps):
        cur = base.step(cur).argmax(-1).astype(np.int32)
        ref.append(cur)
    base.close()
    t = _session(g, smax=96, lm_head=True, kv_dtype="mxfp8")
    d = _session(g_diff, smax=96, lm_head=True)
    toks, _ = SpeculativeDecoder(t, d, k=3).generate(seed_tok, steps)
    np.testing.assert_array_equal(toks, np.stack(ref, axis=1))
    t.close()
    d.close()


def test_mx8_cache_bytes_shapes_and_pool_check(model):
    import torch

    from trtlab_amd.engine.decode import (DecodeSession, PagedKVPool,
                                          kv_row_bytes)

    g, k, _, _, _ = model
    s = _session(g, kv_dtype="mxfp8")
    f = _session(g)
    smax, L = s.smax, s.n_layers
    assert s.kv_cache_bytes == 2 * L * B * k * smax * (HD + HD // 32)
    assert f.kv_cache_bytes == 2 * L * B * k * smax * 2 * HD
    assert s.kv_cache_bytes * 64 == f.kv_cache_bytes * 33
    lay = s.layers[0]
    for name, w in (("kcache", HD), ("vcache", HD), ("kscale", HD // 32),
                    ("vscale", HD // 32)):
        assert lay[name].dtype == torch.uint8, name
        assert tuple(lay[name].shape) == (B, k, smax, w), name
    stored = sum(lay[n].numel() * lay[n].element_size()
                 for n in ("kcache", "vcache", "kscale", "vscale"))
    assert stored * L == s.kv_cache_bytes
    assert f.layers[0]["kcache"].dtype == torch.half
    assert f.layers[0]["kscale"] is None
    s.close()
    f.close()

    p = _session(g, paged=True, kv_dtype="mxfp8")
    pages = B * ((p.smax + 63) // 64)
    pool = p.kv_pool
    assert pool.kv_dtype == "mxfp8"
    assert pool.kpools[0].dtype == torch.uint8
    assert tuple(pool.kpools[0].shape) == (pages, 64, k, HD)
    assert tuple(pool.vpools[0].shape) == (pages, 64, k, HD)
    assert tuple(pool.kscales[0].shape) == (pages, 64, k, HD // 32)
    assert tuple(pool.vscales[0].shape) == (pages, 64, k, HD // 32)
    assert len(pool.kscales) == len(pool.vscales) == L
    assert p.layers[0]["kcache"] is None and p.layers[0]["kscale"] is None
    assert p.kv_cache_bytes == \
        2 * L * pages * 64 * k * kv_row_bytes(HD, "mxfp8")
    p.close()

    half_pool = PagedKVPool(2, k, B, num_pages=4, max_pages_per_slot=2,
                            head_dim=HD)
    assert half_pool.kv_dtype == "fp16" and half_pool.kscales is None
    mx_pool = PagedKVPool(2, k, B, num_pages=4, max_pages_per_slot=2,
                          head_dim=HD, kv_dtype="mxfp8")
    with pytest.raises(ValueError, match="kv_dtype"):
        DecodeSession(g, batch=B, capture=False, paged=half_pool,
                      kv_dtype="mxfp8")
    with pytest.raises(ValueError, match="kv_dtype"):
        DecodeSession(g, batch=B, capture=False, paged=mx_pool)
    DecodeSession(g, batch=B, capture=False, paged=mx_pool,
                  kv_dtype="mxfp8").close()
    with pytest.raises(ValueError):
        PagedKVPool(2, k, B, num_pages=4, max_pages_per_slot=2,
                    head_dim=HD, kv_dtype="fp4")


def test_mx8_rejected_configurations(model):
    from trtlab_amd.engine.decode import DecodeSession

    g = model[0]
    with pytest.raises(ValueError, match="fp16 KV cache"):
        DecodeSession(g, batch=B, lm_head=True, fused=True,
                      kv_dtype="mxfp8")
    with pytest.raises(ValueError, match="kv_dtype"):
        DecodeSession(g, batch=B, kv_dtype="fp8")


def test_mx8_paged_idle_reset_returns_pages(model):
    g, _, toks, _, _ = model
    s = _session(g, paged=True, kv_dtype="mxfp8")
    total = s.kv_pool.pages_free
    s.step(toks[:, 0])
    assert s.kv_pool.pages_free == total - B
    s.idle_slot(1)
    assert s.kv_pool.pages_free == total - B + 1
    s.reset_slot(0)
    assert s.kv_pool.pages_free == total
    out = s.step(toks[:, 1])  # slot 0 restarts at position 0, slot 1 idle
    assert s.kv_pool.pages_free == total - 1
    assert np.isfinite(out[0]).all()
    fresh = _session(g, paged=True, kv_dtype="mxfp8")
    want = fresh.step(toks[:, 1])
    assert np.allclose(out[0], want[0], atol=1e-3)
    s.close()
    fresh.close()
