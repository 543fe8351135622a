"""KV-cache decode ops called directly: kv_append, decode_attention,
decode_embed (csrc/kernels/decode.hip), dense and paged, rows = 1 (step),
3 (verify chunk) and a prefill range.

The session-level tests compare whole models at 2e-2..5e-2, too loose to
notice one wrong cache row or a broken clamp. Here every cache / output
buffer is over-allocated and pre-filled with the sentinel bit pattern
0x7BCD, so both "the right rows were written, bit for bit" and "nothing
else was touched" (idle slot, unmapped pages, guard tail) are checked.

Shape: B = 3 slots (slot 2 idle, pos = -1), H = 2, smax = 192 (three
64-position pages), D in {64, 128}. The paged pool has 12 pages; the block
table is a non-identity permutation, 4 entries per slot with the last -1.

Attention oracle: fp64 softmax(q K^T scale) V on the same fp16 inputs,
atol = 1e-3, rtol = 0, no excluded elements. The output is a convex
combination of V values in [-1, 1] rounded to fp16: half an fp16 ulp below
1.0 is 2^-12 ~ 2.4e-4; fp32 accumulation over <= 130 keys and __expf error
are orders of magnitude below that, so 1e-3 leaves ~4x margin and still
fails a single mis-addressed key (unfilled cache rows hold the sentinel,
fp16 ~6.4e4).
"""
import functools

import numpy as np
import pytest
import torch

import trtlab_amd

pytestmark = pytest.mark.gpu

B, H, SMAX = 3, 2, 192
NPAGES, MAXP = 12, 4
TABLE = np.array([[7, 2, 9, -1], [4, 11, 0, -1], [5, 1, 8, -1]], np.int32)
SENT = 0x7BCD
GUARD = 4096  # sentinel elements after every cache / output
ATOL = 1e-3


@pytest.fixture(scope="module")
def C():
    return trtlab_amd.native()


def _uniform_half(seed, *shape):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(*shape, generator=g) * 2 - 1).half()


def _bits(t):
    return t.contiguous().view(torch.int16).numpy()


def _row_off(layout, table, b, h, t, D):
    """Element offset of row t of (slot b, head h); None if unmapped."""
    if layout == "dense":
        return ((b * H + h) * SMAX + t) * D
    page = int(table[b, t >> 6]) if (t >> 6) < MAXP else -1
    if page < 0:
        return None
    return ((page * 64 + (t & 63)) * H + h) * D


def _cache_elems(layout, D):
    return (B * H * SMAX if layout == "dense" else NPAGES * 64 * H) * D


def _sentinel(elems):
    return np.full(elems, SENT, np.int16)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _paged_args(layout, table):
    if layout == "dense":
        return None, {}
    dt = _dev(table)
    return dt, dict(table=dt.data_ptr(), max_pages=MAXP)


# ------------------------------------------------------------------ append
def _run_append(C, layout, D, rows, pos, table=TABLE):
    """Runs kv_append on sentinel caches. Returns (got_k, got_v, exp_k,
    exp_v, check): int16 host arrays over the whole allocation, and the
    mask of elements whose content is checked (everything except a
    position that several blocks write)."""
    hid = H * D
    qkv = _uniform_half(17 * D + rows, B * rows, 3 * hid)
    qb = _bits(qkv)
    elems = _cache_elems(layout, D) + GUARD
    exp_k, exp_v = _sentinel(elems), _sentinel(elems)
    writers = np.zeros(elems, np.int32)
    for b in range(B):
        if pos is not None and pos[b] < 0:
            continue
        for q in range(rows):
            p = min((pos[b] if pos is not None else 0) + q, SMAX - 1)
            for h in range(H):
                off = _row_off(layout, table, b, h, p, D)
                if off is None:
                    continue
                src = qb[b * rows + q]
                exp_k[off:off + D] = src[hid + h * D:hid + (h + 1) * D]
                exp_v[off:off + D] = src[2 * hid + h * D:2 * hid + (h + 1) * D]
                writers[off:off + D] += 1
    dk, dv, dq = _dev(_sentinel(elems)), _dev(_sentinel(elems)), qkv.cuda()
    dpos = _dev(np.asarray(pos, np.int32)) if pos is not None else None
    dt, kw = _paged_args(layout, table)
    torch.cuda.synchronize()
    C.ops.kv_append(dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), B, H, rows,
                    SMAX, pos=dpos.data_ptr() if dpos is not None else 0,
                    D=D, **kw)
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
@pytest.mark.parametrize("rows", [1, 3])
def test_kv_append(C, rows, layout, D):
    """pos 62 and 127 both cross a page boundary inside a 3-row chunk."""
    res = _run_append(C, layout, D, rows, [62, 127, -1])
    assert res[4].all()  # no position written twice: nothing excluded
    _assert_cache(*res)


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("layout", ["dense", "paged"])
def test_kv_append_range(C, layout, D):
    """Null pos: base position 0 for every slot, the idle one included."""
    res = _run_append(C, layout, D, 70, None)
    assert res[4].all()
    _assert_cache(*res)


@pytest.mark.parametrize("D", [64, 128])
def test_kv_append_unmapped_page_skipped(C, D):
    """Slot 0's second page unmapped: rows at 62, 63 land, row 64 is
    dropped (no write through a negative page id)."""
    table = TABLE.copy()
    table[0, 1] = -1
    res = _run_append(C, "paged", D, 3, [62, 127, -1], table=table)
    assert res[4].all()
    _assert_cache(*res)


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("rows,pos", [(3, [SMAX - 2, 5, -1]), (200, None)])
def test_kv_append_clamped(C, rows, pos, D):
    """Write positions past smax-1 pile up on smax-1 (several blocks write
    it, so its content is the one thing not checked); rows below it are
    exact and the guard tail behind the cache stays untouched."""
    got_k, got_v, exp_k, exp_v, check = _run_append(C, "dense", D, rows, pos)
    base = pos if pos is not None else [0] * B
    clamped = [b for b in range(B) if base[b] >= 0 and base[b] + rows > SMAX]
    unchecked = np.flatnonzero(~check)
    want = np.concatenate([
        np.arange(D) + _row_off("dense", None, b, h, SMAX - 1, D)
        for b in clamped for h in range(H)])
    assert np.array_equal(unchecked, np.sort(want))
    _assert_cache(got_k, got_v, exp_k, exp_v, check)


# --------------------------------------------------------------- attention
@functools.lru_cache(maxsize=None)
def _attn_inputs(D):
    """Logical K/V [B, H, SMAX, D] and a 3-row-per-slot qkv, fp16 on the
    host, shared (read-only) by every attention case of this head_dim."""
    k = _uniform_half(100 + D, B, H, SMAX, D)
    v = _uniform_half(200 + D, B, H, SMAX, D)
    qkv3 = _uniform_half(300 + D, B, 3, 3 * H * D)
    return k, v, qkv3


def _fill_cache(layout, D, src, upto):
    """Sentinel cache with logical rows 0..upto[b]-1 of every head."""
    buf = _sentinel(_cache_elems(layout, D) + GUARD)
    sb = _bits(src).reshape(B, H, SMAX, D)
    for b in range(B):
        for t in range(upto[b]):
            for h in range(H):
                off = _row_off(layout, TABLE, b, h, t, D)
                buf[off:off + D] = sb[b, h, t]
    return buf


def _run_attention(C, layout, D, rows, pos, qsel):
    """qsel: which of the 3 shared query rows per slot the call uses.
    Returns the whole output allocation as int16 [B*rows*hid + GUARD]."""
    hid = H * D
    k, v, qkv3 = _attn_inputs(D)
    qkv = qkv3[:, qsel].reshape(B * rows, 3 * hid)
    upto = [max(p + rows, 0) if p >= 0 else 0 for p in pos]
    dk = _dev(_fill_cache(layout, D, k, upto))
    dv = _dev(_fill_cache(layout, D, v, upto))
    dq = qkv.contiguous().cuda()
    out = _dev(_sentinel(B * rows * hid + GUARD))
    dpos = _dev(np.asarray(pos, np.int32))
    dt, kw = _paged_args(layout, TABLE)
    torch.cuda.synchronize()
    C.ops.decode_attention(dq.data_ptr(), dk.data_ptr(), dv.data_ptr(),
                           out.data_ptr(), dpos.data_ptr(), B, H, rows, SMAX,
                           1.0 / float(np.sqrt(D)), D=D, **kw)
    return out.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _attn_oracle(D, rows, pos, qsel):
    """fp64 reference [B, rows, H*D]; NaN rows for idle slots."""
    k, v, qkv3 = _attn_inputs(D)
    k64, v64 = k.double().numpy(), v.double().numpy()
    q64 = qkv3[:, list(qsel)].double().numpy()
    ref = np.full((B, rows, H * D), np.nan)
    for b in range(B):
        if pos[b] < 0:
            continue
        for q in range(rows):
            n = pos[b] + q + 1
            for h in range(H):
                s = k64[b, h, :n] @ q64[b, q, h * D:(h + 1) * D] / np.sqrt(D)
                e = np.exp(s - s.max())
                ref[b, q, h * D:(h + 1) * D] = (e / e.sum()) @ v64[b, h, :n]
    return ref


def _check_attention(raw, D, rows, pos, qsel):
    hid = H * D
    ref = _attn_oracle(D, rows, tuple(pos), tuple(qsel))
    out = raw[:B * rows * hid].reshape(B, rows, hid)
    assert (raw[B * rows * hid:] == np.int16(SENT)).all(), "guard tail written"
    for b in range(B):
        if pos[b] < 0:
            assert (out[b] == np.int16(SENT)).all(), "idle slot's rows written"
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
@pytest.mark.parametrize("layout", ["dense", "paged"])
@pytest.mark.parametrize("rows", [1, 3])
def test_decode_attention(C, rows, layout, D):
    """n = 1 is the degenerate softmax; n = 128..130 spans three pages and
    leaves lanes with unequal key counts."""
    pos = [0, 127, -1]
    raw = _run_attention(C, layout, D, rows, pos, _QSEL[rows])
    _check_attention(raw, D, rows, pos, _QSEL[rows])


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("rows", [1, 3])
def test_decode_attention_paged_equals_dense(C, rows, D):
    pos = [0, 127, -1]
    dense = _run_attention(C, "dense", D, rows, pos, _QSEL[rows])
    paged = _run_attention(C, "paged", D, rows, pos, _QSEL[rows])
    assert torch.equal(torch.from_numpy(dense), torch.from_numpy(paged))


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("layout", ["dense", "paged"])
def test_decode_attention_step_equals_chunk_row(C, layout, D):
    """rows = 1 at pos = p is bit-equal to row q of a rows = 3 call whose
    pos + q = p (same query row, same keys)."""
    hid = H * D
    chunk = _run_attention(C, layout, D, 3, [0, 127, -1], [0, 1, 2])
    chunk = chunk[:B * 3 * hid].reshape(B, 3, hid)
    for q in range(3):
        step = _run_attention(C, layout, D, 1, [q, 127 + q, -1], [q])
        step = step[:B * hid].reshape(B, hid)
        assert torch.equal(torch.from_numpy(step[:2].copy()),
                           torch.from_numpy(chunk[:2, q].copy())), f"row {q}"


# ------------------------------------------------------------------- embed
@pytest.mark.parametrize("rows", [1, 3])
def test_decode_embed(C, rows):
    hidden, vocab = 64, 50
    pos = [0, SMAX - 2, -1]
    tok = _uniform_half(1, vocab, hidden)
    pe = _uniform_half(2, SMAX, hidden)
    g = torch.Generator().manual_seed(3 + rows)
    ids = torch.randint(0, vocab, (B * rows,), generator=g, dtype=torch.int32)
    exp = _sentinel(B * rows * hidden + GUARD)
    for b in range(B):
        if pos[b] < 0:
            continue
        for q in range(rows):
            r = b * rows + q
            p = min(pos[b] + q, SMAX - 1)
            row = (tok[int(ids[r])].float() + pe[p].float()).half()
            exp[r * hidden:(r + 1) * hidden] = _bits(row)
    out = _dev(_sentinel(exp.size))
    dtok, dpe, dids = tok.cuda(), pe.cuda(), ids.cuda()
    dpos = _dev(np.asarray(pos, np.int32))
    torch.cuda.synchronize()
    C.ops.decode_embed(dids.data_ptr(), dtok.data_ptr(), dpe.data_ptr(),
                       out.data_ptr(), dpos.data_ptr(), B, rows, SMAX, hidden)
    assert torch.equal(out.cpu(), torch.from_numpy(exp))


# ------------------------------------------------------------------ guards
@pytest.mark.parametrize("layout", ["dense", "paged"])
@pytest.mark.parametrize("smax,D", [(4160, 64), (SMAX, 96)])
def test_decode_attention_guards(C, smax, D, layout):
    """smax beyond the 4096-entry LDS score buffer and an unsupported
    head_dim throw in the launcher, before any launch, in both layouts."""
    buf = _dev(_sentinel(GUARD))
    dpos = _dev(np.full(B, -1, np.int32))
    dt, kw = _paged_args(layout, TABLE)
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError):
        C.ops.decode_attention(buf.data_ptr(), buf.data_ptr(), buf.data_ptr(),
                               buf.data_ptr(), dpos.data_ptr(), B, H, 1, smax,
                               0.125, D=D, **kw)
