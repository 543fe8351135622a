"""Top-k / nucleus truncation rule (engine/sampling.py) and its routing
through GenerationEngine. CPU-only: the reference is checked against the
candidate set of GenerationEngine._sample on tie-free rows and against the
value-class rule on tied rows; the engine is driven by a recording fake
session."""
import asyncio

import numpy as np
import pytest

from trtlab_amd.engine.sampling import truncation_reference
from trtlab_amd.rpc.generation import GenerationEngine


def _sample_mask(logits, temperature, top_k, top_p):
    """Candidate set of GenerationEngine._sample (its lines, minus the
    draw): the `keep` most probable tokens."""
    x = logits.astype(np.float64) / temperature
    x -= x.max()
    p = np.exp(x)
    p /= p.sum()
    order = np.argsort(-p)
    keep = len(order)
    if top_k > 0:
        keep = min(keep, top_k)
    if 0.0 < top_p < 1.0:
        keep = min(keep, int(np.searchsorted(np.cumsum(p[order]), top_p) + 1))
    mask = np.zeros(len(order), bool)
    mask[order[:keep]] = True
    return mask


TIE_FREE = (np.random.RandomState(5).permutation(97) * 0.25).astype(np.float16)


@pytest.mark.parametrize("T", [0.7, 1.5])
@pytest.mark.parametrize("top_p", [0, 0.1, 0.5, 0.9, 1.0])
@pytest.mark.parametrize("top_k", [0, 1, 5, 96, 97, 500])
def test_reference_matches_sample_on_tie_free_rows(top_k, top_p, T):
    thr, kept, mask = truncation_reference(TIE_FREE, T, top_k, top_p)
    want = _sample_mask(TIE_FREE.astype(np.float32), T, top_k, top_p)
    np.testing.assert_array_equal(mask, want)
    assert kept == int(want.sum()) == int(mask.sum())
    assert (TIE_FREE.astype(np.float64) >= thr).tolist() == mask.tolist()


def test_reference_small_sets_match_sample_draws():
    """The mask reimplementation above is _sample's: for small sets the
    draws of the real _sample over many seeds cover exactly the set."""
    for top_k, top_p in ((5, 0.0), (0, 0.5), (3, 0.9)):
        _, kept, mask = truncation_reference(TIE_FREE, 1.5, top_k, top_p)
        draws = {GenerationEngine._sample(TIE_FREE.astype(np.float32), 1.5,
                                          top_k, top_p,
                                          np.random.RandomState(i))
                 for i in range(400)}
        assert draws == set(np.flatnonzero(mask).tolist()), (top_k, top_p)


def test_reference_greedy_ignores_filters():
    x = np.array([1.0, 3.0, 3.0, -2.0], np.float16)
    thr, kept, mask = truncation_reference(x, 0.0, 2, 0.5)
    assert (thr, kept, mask.tolist()) == (3.0, 1, [False, True, False, False])


TIED = np.round(np.random.RandomState(4).randn(2, 1000) * 2).astype(np.float16)


def test_ties_keep_the_whole_class():
    thr, kept, mask = truncation_reference(TIED[0], 1.0, 10, 0.0)
    assert (thr, kept) == (4.0, 39)
    np.testing.assert_array_equal(mask, TIED[0] >= 4.0)
    thr, kept, mask = truncation_reference(TIED[1], 1.0, 10, 0.0)
    assert (thr, kept) == (5.0, 13)
    np.testing.assert_array_equal(mask, TIED[1] >= 5.0)


@pytest.mark.parametrize("top_k,top_p", [(10, 0.0), (0, 0.7), (25, 0.5)])
def test_kept_set_is_permutation_invariant(top_k, top_p):
    perm = np.random.RandomState(9).permutation(TIED.shape[1])
    for row in TIED:
        thr, kept, mask = truncation_reference(row, 0.9, top_k, top_p)
        thr2, kept2, mask2 = truncation_reference(row[perm], 0.9, top_k, top_p)
        assert (thr, kept) == (thr2, kept2)
        np.testing.assert_array_equal(mask[perm], mask2)


def test_signed_zeros_share_a_class():
    x = np.array([2.0] + [0.0, -0.0] * 3 + [-1.0] * 4, np.float16)
    thr, kept, mask = truncation_reference(x, 1.0, 2, 0.0)
    assert (thr, kept) == (0.0, 7)
    assert mask.tolist() == [True] * 7 + [False] * 4


def test_neg_inf_rows():
    x = np.array([-np.inf] * 100 + [0.0] * 50 + [-0.0] * 50 + [2.0],
                 np.float16)
    thr, kept, mask = truncation_reference(x, 1.0, 2, 0.0)
    assert (thr, kept) == (0.0, 101)
    # top_k reaching past the finite tokens never keeps a masked one
    thr, kept, mask = truncation_reference(x, 1.0, 150, 0.0)
    assert (thr, kept) == (0.0, 101) and not mask[:100].any()
    # no filter active: nothing is cut
    thr, kept, mask = truncation_reference(x, 1.0, 0, 1.0)
    assert (thr, kept) == (float("-inf"), 201) and mask.all()


# ---- engine routing ----

class RecordingSession:
    """Session fake with both device capabilities. step() refuses to hand
    out logits; sample_tokens() records its arguments and answers with the
    greedy chain token so streams terminate normally."""

    supports_ids = True
    supports_truncation = True

    def __init__(self, batch, logits_ok=False):
        self.batch = batch
        self.smax = 256
        self.logits_ok = logits_ok
        self.logit_steps = 0
        self.id_steps = 0
        self.sample_calls = []
        self._next = np.zeros(batch, np.int32)

    def step(self, ids, return_ids=False):
        self._next = ((7 * np.asarray(ids, np.int64) + 3) % 97).astype(
            np.int32)
        if return_ids:
            self.id_steps += 1
            return self._next.copy()
        assert self.logits_ok, "step() was asked for logits"
        self.logit_steps += 1
        logits = np.zeros((self.batch, 97), np.float32)
        logits[np.arange(self.batch), self._next] = 1.0
        return logits

    def sample_tokens(self, temps, seeds, top_k=None, top_p=None):
        self.sample_calls.append(tuple(
            None if a is None else np.array(a) for a in
            (temps, seeds, top_k, top_p)))
        return self._next.copy()

    def reset_slot(self, b):
        pass

    def idle_slot(self, b):
        pass


STREAMS = (dict(temperature=0.0, seed=0),
           dict(temperature=0.8, top_k=20, seed=11),
           dict(temperature=1.2, top_p=0.9, seed=12))


async def _run_streams(eng, n=4):
    eng.ensure_started()
    subs = [await eng.submit([5 + i], n, **kw)
            for i, kw in enumerate(STREAMS)]
    outs = []
    for b, q in subs:
        toks = []
        while True:
            t = await q.get()
            if t is None:
                break
            toks.append(t)
        outs.append((b, toks))
    await eng.stop()
    return outs


def test_engine_routes_filters_to_device():
    sess = RecordingSession(4)
    eng = GenerationEngine(sess, device_truncation=True)
    outs = asyncio.run(_run_streams(eng))
    assert sess.logit_steps == 0 and sess.id_steps == eng.steps > 0
    assert all(len(toks) == 4 for _, toks in outs)
    slots = [b for b, _ in outs]
    # every step with all three streams live carries their parameters
    full = [c for c in sess.sample_calls if c[2] is not None and
            (c[0][slots] > 0).sum() == 2]
    assert full
    for temps, seeds, top_k, top_p in full:
        assert temps.dtype == np.float32 and top_p.dtype == np.float32
        assert seeds.dtype == np.int32 and top_k.dtype == np.int32
        assert all(a.shape == (4,) for a in (temps, seeds, top_k, top_p))
        np.testing.assert_allclose(temps[slots], [0.0, 0.8, 1.2], rtol=1e-6)
        assert seeds[slots].tolist() == [0, 11, 12]
        assert top_k[slots].tolist() == [0, 20, 0]
        np.testing.assert_allclose(top_p[slots], [0.0, 0.0, 0.9], rtol=1e-6)
        idle = [b for b in range(4) if b not in slots]
        assert not temps[idle].any() and not top_k[idle].any()
        assert not top_p[idle].any()


def test_engine_passes_no_filter_arrays_without_filters():
    """Streams without top_k / top_p keep today's two-argument call even
    with the switch on."""
    sess = RecordingSession(2)
    eng = GenerationEngine(sess, device_truncation=True)

    async def run():
        eng.ensure_started()
        b, q = await eng.submit([5], 3, temperature=0.7, seed=3)
        while await q.get() is not None:
            pass
        await eng.stop()

    asyncio.run(run())
    assert sess.sample_calls
    assert all(c[2] is None and c[3] is None for c in sess.sample_calls)


def test_engine_default_keeps_host_path():
    sess = RecordingSession(4, logits_ok=True)
    eng = GenerationEngine(sess)
    outs = asyncio.run(_run_streams(eng))
    assert all(len(toks) == 4 for _, toks in outs)
    assert sess.logit_steps > 0
    assert all(c[2] is None and c[3] is None for c in sess.sample_calls)


def test_engine_switch_needs_session_capability():
    class NoTrunc(RecordingSession):
        supports_truncation = False

    sess = NoTrunc(4, logits_ok=True)
    eng = GenerationEngine(sess, device_truncation=True)
    asyncio.run(_run_streams(eng))
    assert sess.logit_steps > 0
    assert all(c[2] is None for c in sess.sample_calls)
