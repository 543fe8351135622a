"""Device-side top-k / nucleus sampling (csrc/kernels/sampling.hip) against
the numpy rule in trtlab_amd/engine/sampling.py, from the kernel up through
DecodeSession.sample_tokens and GenerationEngine(device_truncation=True).

The kernel's optional outputs (kept-set size, threshold logit) make the
truncation checkable exactly. Where per-token mass is tiny (V=50257,
top_p=0.999) the cut may legitimately sit one class either way, so those
cases are held to a band: thr_ref(top_p + D) <= thr_dev <= thr_ref(top_p - D)
with D = 1e-5 absolute, which covers the kernel's __expf relative error
(~|z| * 2^-24, a few 1e-6 at |z| <~ 40) plus the fixed-point truncation
(V * 2^-40) with about 3x margin.
"""
import asyncio
import functools

import numpy as np
import pytest

from trtlab_amd.engine.sampling import truncation_reference

pytestmark = pytest.mark.gpu

DELTA = 1e-5
SHAPES = {0: (1000, 3), 1: (257, 3), 2: (7, 3), 3: (50257, 2)}


@functools.lru_cache(maxsize=None)
def _rows(seed):
    V, scale = SHAPES[seed]
    x = (np.random.RandomState(seed).randn(4, V) * scale).astype(np.float16)
    x.setflags(write=False)
    return x


def _f32(v):
    """The value the kernel sees for a float argument."""
    return float(np.float32(v))


def _launch(x, temps, top_k, top_p, seeds=None, pos=None, aux=True):
    """x: fp16 [M, V] numpy array or CUDA tensor (possibly an offset view).
    Returns (out, kept, thr) as numpy arrays (kept/thr None without aux)."""
    import torch

    import trtlab_amd

    C = trtlab_amd.native()
    if isinstance(x, np.ndarray):
        x = torch.from_numpy(np.array(x)).cuda()
    M, V = x.shape

    def dev(a, dt):
        a = np.zeros(M, dt) if a is None else np.ascontiguousarray(a, dt)
        assert a.shape == (M,)
        return torch.from_numpy(a).cuda()

    t, k, p = dev(temps, np.float32), dev(top_k, np.int32), dev(top_p, np.float32)
    s, ps = dev(seeds, np.int32), dev(pos, np.int32)
    out = torch.full((M,), -1, dtype=torch.int32, device="cuda")
    kept = torch.full((M,), -1, dtype=torch.int32, device="cuda")
    thr = torch.full((M,), float("nan"), dtype=torch.float32, device="cuda")
    C.ops.topk_topp_sample_rows(
        x.data_ptr(), out.data_ptr(), temps=t.data_ptr(), top_k=k.data_ptr(),
        top_p=p.data_ptr(), seeds=s.data_ptr(), pos=ps.data_ptr(), M=M, V=V,
        kept=kept.data_ptr() if aux else 0, thr=thr.data_ptr() if aux else 0)
    if not aux:
        return out.cpu().numpy(), None, None
    return out.cpu().numpy(), kept.cpu().numpy(), thr.cpu().numpy()


def _gumbel(x, temps, seeds, pos):
    import torch

    import trtlab_amd

    C = trtlab_amd.native()
    if isinstance(x, np.ndarray):
        x = torch.from_numpy(np.array(x)).cuda()
    M, V = x.shape
    t = torch.from_numpy(np.ascontiguousarray(temps, np.float32)).cuda()
    s = torch.from_numpy(np.ascontiguousarray(seeds, np.int32)).cuda()
    ps = torch.from_numpy(np.ascontiguousarray(pos, np.int32)).cuda()
    out = torch.full((M,), -1, dtype=torch.int32, device="cuda")
    C.ops.gumbel_argmax_rows(x.data_ptr(), out.data_ptr(), temps=t.data_ptr(),
                             seeds=s.data_ptr(), pos=ps.data_ptr(), M=M, V=V)
    return out.cpu().numpy()


def _grid(rows, Ts, ks, ps):
    """Every row under every (T, top_k, top_p): tiled rows + per-row args."""
    xs, T, K, P = [], [], [], []
    for t in Ts:
        for k in ks:
            for p in ps:
                for r in rows:
                    xs.append(r)
                    T.append(t)
                    K.append(k)
                    P.append(p)
    return (np.stack(xs), np.array(T, np.float32), np.array(K, np.int32),
            np.array(P, np.float32))


def _assert_banded(row, T, k, p, thr_dev, kept_dev):
    """thr_dev within the reference band around top_p; kept consistent."""
    T, p = _f32(T), _f32(p)
    if 0.0 < p < 1.0:
        lo = truncation_reference(row, T, k, p + DELTA)[0]
        hi = truncation_reference(row, T, k, p - DELTA)[0]
    else:
        lo = hi = truncation_reference(row, T, k, p)[0]
    assert lo <= thr_dev <= hi, (T, k, p, lo, thr_dev, hi)
    x = row.astype(np.float64) + 0.0
    assert kept_dev == int((x >= thr_dev).sum()), (T, k, p, thr_dev, kept_dev)
    return x >= thr_dev


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_truncation_exact(seed):
    x, T, K, P = _grid(_rows(seed), [0.7, 1.0, 1.5], [0, 1, 5, 50],
                       [0, 0.1, 0.5, 0.9])
    out, kept, thr = _launch(x, T, K, P, seeds=np.arange(len(T)))
    for i in range(len(T)):
        t, k, p = _f32(T[i]), int(K[i]), _f32(P[i])
        rthr, rkept, mask = truncation_reference(x[i], t, k, p)
        if 0.0 < p < 1.0:
            # precondition, from the reference itself: no class boundary's
            # cumulative mass lies within 1e-4 of top_p, so device rounding
            # (orders of magnitude smaller) cannot move the cut
            assert truncation_reference(x[i], t, k, p + 1e-4)[0] == rthr
            assert truncation_reference(x[i], t, k, p - 1e-4)[0] == rthr
        assert (thr[i], kept[i]) == (rthr, rkept), (i, t, k, p)
        assert mask[out[i]], (i, t, k, p, out[i])


def test_truncation_banded_large_vocab():
    x, T, K, P = _grid(_rows(3), [0.7, 1.0, 1.5], [0, 50],
                       [0.1, 0.5, 0.9, 0.999])
    out, kept, thr = _launch(x, T, K, P, seeds=np.arange(len(T)))
    for i in range(len(T)):
        mask = _assert_banded(x[i], T[i], int(K[i]), P[i], thr[i], kept[i])
        assert mask[out[i]]


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_truncation_banded_wide_nucleus(seed):
    x, T, K, P = _grid(_rows(seed), [0.7, 1.0, 1.5], [0, 50], [0.999])
    out, kept, thr = _launch(x, T, K, P, seeds=np.arange(len(T)))
    for i in range(len(T)):
        mask = _assert_banded(x[i], T[i], int(K[i]), P[i], thr[i], kept[i])
        assert mask[out[i]]


def test_corner_rows():
    # one class is the whole row, and its count does not fit 16 bits
    ones = np.ones((2, 70000), np.float16)
    out, kept, thr = _launch(ones, [1.0, 1.0], [1, 0], [0.0, 0.5], seeds=[3, 4])
    assert kept.tolist() == [70000, 70000] and thr.tolist() == [1.0, 1.0]
    assert ((0 <= out) & (out < 70000)).all()

    # masked tokens and signed zeros: top_k=2 cuts inside the zero class
    row = np.array([-np.inf] * 100 + [0.0] * 50 + [-0.0] * 50 + [2.0],
                   np.float16)[None]
    out, kept, thr = _launch(row, [1.0], [2], [0.0], seeds=[5])
    assert (kept[0], thr[0]) == (101, 0.0) and out[0] >= 100
    assert truncation_reference(row[0], 1.0, 2, 0.0)[:2] == (0.0, 101)
    # a top_k past the finite tokens never reaches the masked ones
    out, kept, thr = _launch(row, [1.0], [150], [0.0], seeds=[5])
    assert (kept[0], thr[0]) == (101, 0.0) and out[0] >= 100


def test_inactive_filters_are_noops():
    x = np.tile(_rows(0), (3, 1))  # 12 rows, V=1000 < 5000
    M = len(x)
    T = np.full(M, 0.9, np.float32)
    K = np.repeat([5000, 0, 0], 4)
    P = np.repeat([0.0, 1.0, 0.0], 4)
    seeds, pos = np.arange(M) + 100, np.arange(M) * 3
    out, kept, thr = _launch(x, T, K, P, seeds, pos)
    np.testing.assert_array_equal(out, _gumbel(x, T, seeds, pos))
    assert (kept == 1000).all() and np.isneginf(thr).all()
    out2, _, _ = _launch(x, T, K, P, seeds, pos, aux=False)  # null outputs
    np.testing.assert_array_equal(out2, out)


@pytest.mark.parametrize("seed", [0, 3])
def test_odd_row_base(seed):
    """x as a view one element into an over-allocated buffer: every row
    base is 2-byte aligned only (V=1000), or rows alternate (V=50257)."""
    import torch

    x = _rows(seed)
    M, V = x.shape
    T = np.array([0.7, 1.0, 1.5, 0.0], np.float32)
    K = np.array([5, 0, 50, 7], np.int32)
    P = np.array([0.0, 0.5, 0.9, 0.3], np.float32)
    seeds = np.arange(M) + 9
    want = _launch(x, T, K, P, seeds)
    buf = torch.zeros(M * V + 16, dtype=torch.float16, device="cuda")
    for off in (1, 3):
        view = buf[off:off + M * V].view(M, V)
        view.copy_(torch.from_numpy(np.array(x)))
        assert view.data_ptr() % 16 == 2 * off
        got = _launch(view, T, K, P, seeds)
        for g, w in zip(got, want):
            np.testing.assert_array_equal(g, w)


def test_filters_off_equals_gumbel_argmax_rows():
    M, V = 64, 1000
    x = (np.random.RandomState(11).randn(M, V) * 3).astype(np.float16)
    T = np.where(np.arange(M) % 4 == 0, 0.0,
                 0.5 + 0.05 * np.arange(M)).astype(np.float32)
    seeds = np.arange(M) * 7 + 1
    pos = (np.arange(M) * 13) % 97
    out, kept, thr = _launch(x, T, None, None, seeds, pos)
    np.testing.assert_array_equal(out, _gumbel(x, T, seeds, pos))
    greedy = T <= 0
    np.testing.assert_array_equal(out[greedy], x[greedy].argmax(-1))
    assert (kept[greedy] == 1).all() and (kept[~greedy] == V).all()
    np.testing.assert_array_equal(thr[greedy],
                                  x[greedy].max(-1).astype(np.float32))


@pytest.mark.parametrize("top_k,top_p", [(3, 0.0), (0, 0.6)])
def test_draw_frequencies(top_k, top_p):
    """4096 independent draws (one seed per row) from the 8-logit row of
    test_gumbel_argmax_sampling: all inside the kept set, frequencies
    within its 0.03 max-abs bound of the renormalised softmax."""
    M = 4096
    row = np.log(np.array([1, 2, 4, 8, 1, 1, 1, 2], np.float64)).astype(
        np.float16)
    x = np.tile(row, (M, 1))
    out, kept, thr = _launch(x, np.ones(M), np.full(M, top_k),
                             np.full(M, top_p), seeds=np.arange(M))
    assert (kept == kept[0]).all() and (thr == thr[0]).all()
    # top_p=0.6 sits on a class boundary of this row (0.4 + 0.2): the band
    # decides which side is legitimate, the draws must follow the device's
    mask = _assert_banded(row, 1.0, top_k, top_p, thr[0], kept[0])
    assert mask[out].all()
    p = np.exp(row.astype(np.float64)) * mask
    p /= p.sum()
    freq = np.bincount(out, minlength=8) / M
    assert np.abs(freq - p).max() < 0.03, (freq, p)


def _mixed_batch():
    x = np.tile(_rows(0), (2, 1))[:5]
    T = np.array([0.0, 0.8, 0.8, 1.2, 0.7], np.float32)
    K = np.array([0, 0, 20, 0, 40], np.int32)
    P = np.array([0.0, 0.0, 0.0, 0.8, 0.9], np.float32)
    return x, T, K, P, np.arange(5) + 21, np.array([0, 4, 9, 2, 30])


def test_deterministic():
    x, T, K, P, seeds, pos = _mixed_batch()
    first = _launch(x, T, K, P, seeds, pos)
    for _ in range(19):
        for g, w in zip(_launch(x, T, K, P, seeds, pos), first):
            np.testing.assert_array_equal(g, w)


def test_mixed_batch_rows_are_independent():
    """greedy / temperature-only / top-k / top-p / both in one launch: each
    row's truncation equals the row launched alone, and its token equals
    the launch with every OTHER row switched to greedy (the noise key holds
    the row index, so the row keeps its place for the token check)."""
    x, T, K, P, seeds, pos = _mixed_batch()
    out, kept, thr = _launch(x, T, K, P, seeds, pos)
    for i in range(5):
        _, k1, t1 = _launch(x[i:i + 1], T[i:i + 1], K[i:i + 1], P[i:i + 1],
                            seeds[i:i + 1], pos[i:i + 1])
        assert (k1[0], t1[0]) == (kept[i], thr[i])
        only = np.arange(5) == i
        o2, k2, t2 = _launch(x, T * only, K * only, P * only, seeds, pos)
        assert (o2[i], k2[i], t2[i]) == (out[i], kept[i], thr[i])
        others = ~only
        np.testing.assert_array_equal(o2[others], x[others].argmax(-1))


# ---- DecodeSession / GenerationEngine ----

def _llama_session(**kw):
    from trtlab_amd.engine.decode import DecodeSession
    from trtlab_amd.models import build_llama

    g = build_llama(batch=2, seq=32, hidden=256, layers=2, heads=4, seed=0,
                    vocab=1000)
    return DecodeSession(g, batch=2, smax=32, lm_head=True, **kw)


def _in_banded_set(row, T, k, p, tok):
    """tok lies in the widest kept set the band allows for (T, k, p)."""
    T, p = _f32(T), _f32(p)
    if T <= 0.0:
        return tok == int(np.argmax(row))
    pp = p + DELTA if 0.0 < p < 1.0 else p
    return bool(truncation_reference(row, T, k, pp)[2][tok])


@pytest.mark.parametrize("paged", [False, True])
def test_session_sample_tokens_truncation(paged):
    s = _llama_session(capture=False, paged=paged)
    assert s.supports_truncation
    s.step(np.array([5, 9], np.int32), return_ids=True)
    t = np.full(2, 1.5, np.float32)
    sd = np.array([7, 8], np.int32)
    plain = s.sample_tokens(t, sd)
    np.testing.assert_array_equal(s.sample_tokens(t, sd, None, None), plain)
    np.testing.assert_array_equal(  # inactive filters: the same draw
        s.sample_tokens(t, sd, np.zeros(2, np.int32), np.zeros(2, np.float32)),
        plain)
    K = np.array([1, 0], np.int32)
    P = np.array([0.0, 0.5], np.float32)
    a = s.sample_tokens(t, sd, top_k=K, top_p=P)
    b = s.sample_tokens(t, sd, top_k=K, top_p=P)
    np.testing.assert_array_equal(a, b)  # same (seed, pos) -> same draw
    logits = s.logits.cpu().numpy()
    for i in range(2):
        assert _in_banded_set(logits[i], 1.5, int(K[i]), P[i], int(a[i]))
    assert a[0] == logits[0].argmax()  # top_k=1 is the argmax
    s.close()


def test_engine_device_truncation_real_session():
    from trtlab_amd.rpc.generation import GenerationEngine

    prompts = ([7, 101, 33], [4, 250, 19])
    params = (dict(temperature=0.0),
              dict(temperature=1.0, top_k=8, top_p=0.9, seed=7))
    n = 6

    async def run(sess):
        eng = GenerationEngine(sess, device_truncation=True, inline_step=True)
        assert eng.device_truncation
        # queue both before the loop starts: inline steps never yield, so
        # both streams are admitted together and run in lockstep
        subs = [asyncio.ensure_future(eng.submit(p, n, **kw))
                for p, kw in zip(prompts, params)]
        await asyncio.sleep(0)
        eng.ensure_started()
        outs = []
        for sub in subs:
            b, q = await sub
            toks = []
            while True:
                t = await q.get()
                if t is None:
                    break
                toks.append(t)
            outs.append((b, toks))
        await eng.stop()
        return outs

    sess = _llama_session()
    real_step = sess.step

    def ids_only_step(ids, return_ids=False):
        assert return_ids, "a logits row left the GPU"
        return real_step(ids, return_ids=True)

    sess.step = ids_only_step
    outs = asyncio.run(run(sess))
    again = asyncio.run(run(sess))  # same seed => same stream
    sess.close()
    assert outs == again
    assert all(len(toks) == n for _, toks in outs)
    assert sorted(b for b, _ in outs) == [0, 1]

    # replay both streams through an identical session, slot for slot
    ref = _llama_session()
    feeds = {b: list(p) + toks for (b, toks), p in zip(outs, prompts)}
    ids = np.zeros(2, np.int32)
    for step in range(len(prompts[0]) + n - 1):
        for b in (0, 1):
            ids[b] = feeds[b][step]
        lg = ref.step(ids).astype(np.float16)
        if step < len(prompts[0]) - 1:
            continue  # still feeding the prompt
        for (b, toks), kw in zip(outs, params):
            tok = toks[step - (len(prompts[0]) - 1)]
            assert _in_banded_set(lg[b], kw["temperature"],
                                  kw.get("top_k", 0), kw.get("top_p", 0.0),
                                  tok), (step, b, tok)
    ref.close()
