"""Grouped-query attention at the kernel level: kv_append,
decode_attention, rope and the full-sequence attention called directly
with kv_heads (Hq query heads over Hkv kv heads, G = Hq / Hkv).

Method of tests/test_decode_kernels_gpu.py: every cache / output buffer
is over-allocated and pre-filled with the sentinel bit pattern 0x7BCD, so
"the right rows were written, bit for bit" and "nothing else was touched"
(idle slot, unmapped pages, guard tail) are both checked. B = 3 slots
(slot 2 idle, pos = -1), smax = 192, a 12-page pool behind a non-identity
block table whose last entry per slot is -1, inputs uniform in [-1, 1].

Two references:
  * the MHA kernels themselves on the explicitly replicated problem
    (3*Hq*D-wide qkv, caches with every kv head copied across its query
    group). GQA changes addresses only, and each wave of the grouped
    decode kernel runs the MHA per-wave body, so outputs are BIT-equal.
  * for decode_attention also the fp64 oracle, atol = 1e-3, rtol = 0, no
    excluded elements: the output is a convex combination of V values in
    [-1, 1] rounded to fp16 (half an ulp below 1.0 is 2^-12 ~ 2.4e-4);
    fp32 accumulation over <= 4096 keys (~4096 * 2^-24 ~ 2.4e-4 worst
    case, far less in practice) and __expf error stay below that bound.
"""
import functools

import numpy as np
import pytest
import torch

import trtlab_amd

pytestmark = pytest.mark.gpu

B, SMAX = 3, 192
NPAGES, MAXP = 12, 4
TABLE = np.array([[7, 2, 9, -1], [4, 11, 0, -1], [5, 1, 8, -1]], np.int32)
SENT = 0x7BCD
GUARD = 4096
ATOL = 1e-3
HEADS = [(4, 2), (4, 1), (8, 1)]  # (Hq, Hkv)


@pytest.fixture(scope="module")
def C():
    return trtlab_amd.native()


def _uniform_half(seed, *shape):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(*shape, generator=g) * 2 - 1).half()


def _bits(t):
    return t.contiguous().view(torch.int16).numpy()


def _sentinel(elems):
    return np.full(elems, SENT, np.int16)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _paged_args(layout):
    if layout == "dense":
        return None, {}
    dt = _dev(TABLE)
    return dt, dict(table=dt.data_ptr(), max_pages=MAXP)


def _row_off(layout, b, h, t, H, D, smax=SMAX):
    """Element offset of row t of (slot b, cache head h) in a cache that
    holds H heads; None if the page is unmapped."""
    if layout == "dense":
        return ((b * H + h) * smax + t) * D
    page = int(TABLE[b, t >> 6]) if (t >> 6) < MAXP else -1
    if page < 0:
        return None
    return ((page * 64 + (t & 63)) * H + h) * D


def _cache_elems(layout, H, D):
    return (B * H * SMAX if layout == "dense" else NPAGES * 64 * H) * D


def _expand_qkv(qkv, Hq, Hkv, D):
    """[M, (Hq+2Hkv)*D] -> the MHA row [M, 3*Hq*D]: every kv head's k and
    v block repeated across its query group."""
    m = qkv.shape[0]
    G = Hq // Hkv
    x = qkv.reshape(m, Hq + 2 * Hkv, D)
    q, k, v = x[:, :Hq], x[:, Hq:Hq + Hkv], x[:, Hq + Hkv:]
    return torch.cat([q, k.repeat_interleave(G, 1),
                      v.repeat_interleave(G, 1)], 1).reshape(m, 3 * Hq * D) \
        .contiguous()


# ------------------------------------------------------------------ append
def _run_append(C, layout, Hq, Hkv, D, rows, pos):
    W = (Hq + 2 * Hkv) * D
    qkv = _uniform_half(17 * D + rows + Hq * 7 + Hkv, B * rows, W)
    qb = _bits(qkv)
    elems = _cache_elems(layout, Hkv, D) + GUARD
    exp_k, exp_v = _sentinel(elems), _sentinel(elems)
    writers = np.zeros(elems, np.int32)
    for b in range(B):
        if pos is not None and pos[b] < 0:
            continue
        for q in range(rows):
            p = min((pos[b] if pos is not None else 0) + q, SMAX - 1)
            for h in range(Hkv):
                off = _row_off(layout, b, h, p, Hkv, D)
                if off is None:
                    continue
                src = qb[b * rows + q]
                ko = (Hq + h) * D
                vo = (Hq + Hkv + h) * D
                exp_k[off:off + D] = src[ko:ko + D]
                exp_v[off:off + D] = src[vo:vo + D]
                writers[off:off + D] += 1
    dk, dv, dq = _dev(_sentinel(elems)), _dev(_sentinel(elems)), qkv.cuda()
    dpos = _dev(np.asarray(pos, np.int32)) if pos is not None else None
    dt, kw = _paged_args(layout)
    torch.cuda.synchronize()
    C.ops.kv_append(dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), B, Hq, rows,
                    SMAX, pos=dpos.data_ptr() if dpos is not None else 0,
                    D=D, kv_heads=Hkv, **kw)
    return dk.cpu().numpy(), dv.cpu().numpy(), exp_k, exp_v, writers <= 1


def _assert_cache(got_k, got_v, exp_k, exp_v, check):
    for name, got, exp in (("K", got_k, exp_k), ("V", got_v, exp_v)):
        bad = (got != exp) & check
        print(f"{name}: {int((exp != np.int16(SENT)).sum())} written "
              f"elements expected, {int(bad.sum())} mismatches")
        assert not bad.any(), (
            f"{name} cache: {int(bad.sum())} elements differ, first at "
            f"{int(np.flatnonzero(bad)[0])}")


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("layout", ["dense", "paged"])
@pytest.mark.parametrize("heads", HEADS)
@pytest.mark.parametrize("rows,pos", [(1, [62, 127, -1]), (3, [62, 127, -1]),
                                      (70, None)])
def test_kv_append(C, rows, pos, heads, layout, D):
    """rows 1 and 3 at positions crossing a page boundary, and a prefill
    range from a null pos. No position is written twice here."""
    res = _run_append(C, layout, *heads, D, rows, pos)
    assert res[4].all()
    _assert_cache(*res)


@pytest.mark.parametrize("heads", HEADS)
def test_kv_append_clamped(C, heads):
    """A chunk running past smax piles up on position smax-1 of slot 0:
    that row (every kv head) is the only content not checked."""
    Hq, Hkv = heads
    D = 64
    got_k, got_v, exp_k, exp_v, check = _run_append(
        C, "dense", Hq, Hkv, D, 3, [SMAX - 2, 5, -1])
    want = np.concatenate([
        np.arange(D) + _row_off("dense", 0, h, SMAX - 1, Hkv, D)
        for h in range(Hkv)])
    assert np.array_equal(np.flatnonzero(~check), np.sort(want))
    _assert_cache(got_k, got_v, exp_k, exp_v, check)


# --------------------------------------------------------------- attention
@functools.lru_cache(maxsize=None)
def _attn_inputs(Hq, Hkv, D):
    """Logical K/V [B, Hkv, SMAX, D] and a 3-row-per-slot grouped qkv."""
    s = Hq * 1000 + Hkv * 100 + D
    k = _uniform_half(1 + s, B, Hkv, SMAX, D)
    v = _uniform_half(2 + s, B, Hkv, SMAX, D)
    qkv3 = _uniform_half(3 + s, B, 3, (Hq + 2 * Hkv) * D)
    return k, v, qkv3


def _fill_cache(layout, src, upto):
    """Sentinel cache holding logical rows 0..upto[b]-1 of every head of
    src [B, H, SMAX, D]."""
    _, H, _, D = src.shape
    buf = _sentinel(_cache_elems(layout, H, D) + GUARD)
    sb = _bits(src).reshape(B, H, SMAX, D)
    for b in range(B):
        for t in range(upto[b]):
            for h in range(H):
                off = _row_off(layout, b, h, t, H, D)
                buf[off:off + D] = sb[b, h, t]
    return buf


def _run_attention(C, layout, Hq, Hkv, D, rows, pos, qsel, mode="gqa"):
    """mode: "gqa" (kv_heads=Hkv), "mha" (the replicated problem through
    the MHA path, kv_heads omitted), "explicit" (replicated problem with
    kv_heads=Hq spelled out). Returns the whole output allocation."""
    hid = Hq * D
    k, v, qkv3 = _attn_inputs(Hq, Hkv, D)
    qkv = qkv3[:, qsel].reshape(B * rows, -1)
    kw2 = dict(kv_heads=Hkv)
    if mode != "gqa":
        G = Hq // Hkv
        k, v = k.repeat_interleave(G, 1), v.repeat_interleave(G, 1)
        qkv = _expand_qkv(qkv, Hq, Hkv, D)
        kw2 = dict(kv_heads=Hq) if mode == "explicit" else {}
    upto = [max(p + rows, 0) if p >= 0 else 0 for p in pos]
    dk = _dev(_fill_cache(layout, k, upto))
    dv = _dev(_fill_cache(layout, v, upto))
    dq = qkv.contiguous().cuda()
    out = _dev(_sentinel(B * rows * hid + GUARD))
    dpos = _dev(np.asarray(pos, np.int32))
    dt, kw = _paged_args(layout)
    torch.cuda.synchronize()
    C.ops.decode_attention(dq.data_ptr(), dk.data_ptr(), dv.data_ptr(),
                           out.data_ptr(), dpos.data_ptr(), B, Hq, rows, SMAX,
                           1.0 / float(np.sqrt(D)), D=D, **kw, **kw2)
    return out.cpu().numpy()


def _oracle(k, v, q, Hq, Hkv, D, pos, rows):
    """fp64 grouped attention. k, v [B, Hkv, S, D]; q [B, rows, >=Hq*D]
    (q block first). NaN rows for idle slots."""
    nb = k.shape[0]
    G = Hq // Hkv
    k64, v64, q64 = (a.double().numpy() for a in (k, v, q))
    ref = np.full((nb, rows, Hq * D), np.nan)
    for b in range(nb):
        if pos[b] < 0:
            continue
        for r in range(rows):
            n = pos[b] + r + 1
            for h in range(Hq):
                s = k64[b, h // G, :n] @ q64[b, r, h * D:(h + 1) * D] \
                    / np.sqrt(D)
                e = np.exp(s - s.max())
                ref[b, r, h * D:(h + 1) * D] = (e / e.sum()) @ \
                    v64[b, h // G, :n]
    return ref


def _check_oracle(raw, ref, nb, rows, hid, pos):
    out = raw[:nb * rows * hid].reshape(nb, rows, hid)
    assert (raw[nb * rows * hid:] == np.int16(SENT)).all(), \
        "guard tail written"
    for b in range(nb):
        if pos[b] < 0:
            assert (out[b] == np.int16(SENT)).all(), \
                "idle slot's rows written"
            continue
        got = out[b].view(np.float16).astype(np.float64)
        err = np.abs(got - ref[b])
        print(f"slot {b}: n = {pos[b] + 1}..{pos[b] + rows}, "
              f"max err {err.max():.3g}")
        assert (err <= ATOL).all(), (  # NaN compares false
            f"slot {b}: {int((~(err <= ATOL)).sum())} elements out of "
            f"tolerance, max err {np.nanmax(err):.3g}")


_QSEL = {1: [0], 3: [0, 1, 2]}


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("heads", HEADS)
@pytest.mark.parametrize("rows", [1, 3])
def test_decode_attention(C, rows, heads, D):
    """n = 1 is the degenerate softmax; n = 128..130 spans three pages and
    leaves lanes with unequal key counts. Dense and paged against the
    oracle; paged == dense and GQA == MHA-on-replicated bit for bit."""
    Hq, Hkv = heads
    pos = [0, 127, -1]
    qsel = _QSEL[rows]
    k, v, qkv3 = _attn_inputs(Hq, Hkv, D)
    ref = _oracle(k, v, qkv3[:, qsel], Hq, Hkv, D, pos, rows)
    dense = _run_attention(C, "dense", Hq, Hkv, D, rows, pos, qsel)
    paged = _run_attention(C, "paged", Hq, Hkv, D, rows, pos, qsel)
    _check_oracle(dense, ref, B, rows, Hq * D, pos)
    _check_oracle(paged, ref, B, rows, Hq * D, pos)
    assert np.array_equal(dense, paged), "paged != dense"
    for layout, got in (("dense", dense), ("paged", paged)):
        mha = _run_attention(C, layout, Hq, Hkv, D, rows, pos, qsel, "mha")
        assert np.array_equal(got, mha), \
            f"{layout}: GQA differs from MHA on the replicated cache"


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("layout", ["dense", "paged"])
def test_decode_attention_explicit_kv_heads_is_mha(C, layout, D):
    """kv_heads = Hq spelled out == omitting it, bit for bit."""
    pos = [0, 127, -1]
    a = _run_attention(C, layout, 4, 2, D, 3, pos, _QSEL[3], "mha")
    b = _run_attention(C, layout, 4, 2, D, 3, pos, _QSEL[3], "explicit")
    assert np.array_equal(a, b)


def test_decode_attention_g8_full_window(C):
    """G = 8 at smax = 4096: the 128 KiB score buffer must launch, and
    the longest window the kernel supports stays within the oracle bound."""
    Hq, Hkv, D, smax = 8, 1, 64, 4096
    k = _uniform_half(71, 1, Hkv, smax, D)
    v = _uniform_half(72, 1, Hkv, smax, D)
    qkv = _uniform_half(73, 1, 1, (Hq + 2 * Hkv) * D)
    pos = [smax - 1]
    ref = _oracle(k, v, qkv, Hq, Hkv, D, pos, 1)
    dk = _dev(np.concatenate([_bits(k).reshape(-1), _sentinel(GUARD)]))
    dv = _dev(np.concatenate([_bits(v).reshape(-1), _sentinel(GUARD)]))
    dq = qkv.reshape(1, -1).cuda()
    out = _dev(_sentinel(Hq * D + GUARD))
    dpos = _dev(np.asarray(pos, np.int32))
    torch.cuda.synchronize()
    C.ops.decode_attention(dq.data_ptr(), dk.data_ptr(), dv.data_ptr(),
                           out.data_ptr(), dpos.data_ptr(), 1, Hq, 1, smax,
                           1.0 / float(np.sqrt(D)), D=D, kv_heads=Hkv)
    _check_oracle(out.cpu().numpy(), ref, 1, 1, Hq * D, pos)


@pytest.mark.parametrize("layout", ["dense", "paged"])
@pytest.mark.parametrize("heads", [(4, 3), (6, 1)])
def test_decode_attention_guards(C, heads, layout):
    """heads not a multiple of kv_heads, and a group size outside
    {1,2,4,8}, throw in the launcher before any launch."""
    Hq, Hkv = heads
    buf = _dev(_sentinel(GUARD))
    dpos = _dev(np.full(B, -1, np.int32))
    dt, kw = _paged_args(layout)
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError):
        C.ops.decode_attention(buf.data_ptr(), buf.data_ptr(), buf.data_ptr(),
                               buf.data_ptr(), dpos.data_ptr(), B, Hq, 1,
                               SMAX, 0.125, D=64, kv_heads=Hkv, **kw)
    torch.cuda.synchronize()
    assert (buf.cpu().numpy() == np.int16(SENT)).all()


@pytest.mark.parametrize("op", ["rope", "kv_append", "attention"])
def test_other_launchers_reject_bad_kv_heads(C, op):
    buf = _dev(_sentinel(GUARD))
    dpos = _dev(np.full(B, -1, np.int32))
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError):
        if op == "rope":
            C.ops.rope(0, buf.data_ptr(), pos=dpos.data_ptr(), M=B, S=SMAX,
                       H=4, D=64, kv_heads=3)
        elif op == "kv_append":
            C.ops.kv_append(buf.data_ptr(), buf.data_ptr(), buf.data_ptr(),
                            B, 4, 1, SMAX, pos=dpos.data_ptr(), D=64,
                            kv_heads=3)
        else:
            C.ops.attention(0, buf.data_ptr(), buf.data_ptr(), 1, 1, 4, 64,
                            0.125, kv_heads=8)
    torch.cuda.synchronize()
    assert (buf.cpu().numpy() == np.int16(SENT)).all()


# -------------------------------------------------------------------- rope
def _rope_both(C, Hq, Hkv, D, M, **kw):
    """Runs rope on a grouped row and on its MHA expansion (today's
    kernel: kv_heads omitted). Returns (before, after, mha_after) as int16
    [M, width] host arrays plus the grouped buffer's guard tail."""
    W = (Hq + 2 * Hkv) * D
    qkv = _uniform_half(900 + Hq * 10 + Hkv + D + M, M, W)
    buf = _dev(np.concatenate([_bits(qkv).reshape(-1), _sentinel(GUARD)]))
    mha = _expand_qkv(qkv, Hq, Hkv, D).cuda()
    torch.cuda.synchronize()
    C.ops.rope(0, buf.data_ptr(), M=M, H=Hq, D=D, theta=10000.0,
               kv_heads=Hkv, **kw)
    C.ops.rope(0, mha.data_ptr(), M=M, H=Hq, D=D, theta=10000.0, **kw)
    got = buf.cpu().numpy()
    return (_bits(qkv), got[:M * W].reshape(M, W), _bits(mha.cpu()),
            got[M * W:])


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("heads", HEADS)
@pytest.mark.parametrize("mode", ["full", "pos", "chunk"])
def test_rope(C, mode, heads, D):
    """Full-sequence, device-pos with an idle slot, and chunk = 3. q and
    every k head bit-equal to the MHA kernel on the expanded row; v and
    the guard tail bit-unchanged."""
    Hq, Hkv = heads
    G = Hq // Hkv
    if mode == "full":
        M, kw, idle_rows = B * 5, dict(S=5), []
    else:
        dpos = _dev(np.asarray([5, 130, -1], np.int32))
        if mode == "pos":
            M, kw, idle_rows = B, dict(pos=dpos.data_ptr(), S=SMAX), [2]
        else:
            M, idle_rows = B * 3, [6, 7, 8]
            kw = dict(pos=dpos.data_ptr(), S=SMAX, chunk=3)
    before, after, mha, guard = _rope_both(C, Hq, Hkv, D, M, **kw)
    assert (guard == np.int16(SENT)).all(), "guard tail written"
    qw = Hq * D
    assert np.array_equal(after[:, :qw], mha[:, :qw]), "q block"
    for h in range(Hkv):
        assert np.array_equal(
            after[:, qw + h * D:qw + (h + 1) * D],
            mha[:, qw + h * G * D:qw + (h * G + 1) * D]), f"k head {h}"
    assert np.array_equal(after[:, qw + Hkv * D:], before[:, qw + Hkv * D:]), \
        "v block changed"
    live = [r for r in range(M) if r not in idle_rows]
    assert not np.array_equal(after[live, :qw], before[live, :qw]), \
        "rope did nothing"
    assert np.array_equal(after[idle_rows], before[idle_rows]), \
        "idle slot's rows changed"


# ---------------------------------------------------- full-sequence attention
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("heads", HEADS)
@pytest.mark.parametrize("case", ["plain", "causal", "seqlens"])
def test_attention(C, case, heads, D):
    """S = 192: one full 128-key tile plus a tail (D = 64), three 64-key
    tiles (D = 128). Bit-equal to the MHA kernel on the expanded qkv."""
    Hq, Hkv = heads
    nb, S = 2, 192
    M, hid = nb * S, Hq * D
    qkv = _uniform_half(500 + Hq * 10 + Hkv + D, M, (Hq + 2 * Hkv) * D)
    dq = qkv.cuda()
    dm = _expand_qkv(qkv, Hq, Hkv, D).cuda()
    out = _dev(_sentinel(M * hid + GUARD))
    ref = _dev(_sentinel(M * hid + GUARD))
    kw = dict(causal=1 if case == "causal" else 0)
    if case == "seqlens":
        lens = _dev(np.asarray([192, 77], np.int32))
        kw["seqlens"] = lens.data_ptr()
    torch.cuda.synchronize()
    scale = 1.0 / float(np.sqrt(D))
    C.ops.attention(0, dq.data_ptr(), out.data_ptr(), nb, S, Hq, D, scale,
                    kv_heads=Hkv, **kw)
    C.ops.attention(0, dm.data_ptr(), ref.data_ptr(), nb, S, Hq, D, scale,
                    **kw)
    got, exp = out.cpu().numpy(), ref.cpu().numpy()
    assert (got[M * hid:] == np.int16(SENT)).all(), "guard tail written"
    assert (got[:M * hid] != np.int16(SENT)).any()
    assert np.array_equal(got, exp)
