"""MXFP8 KV cache at the kernel level: kv_append and decode_attention
called directly with kv_format=1 (e4m3 code bytes in the cache buffers,
one e8m0 scale byte per 32 elements in kscale / vscale).

Method and constants of tests/test_gqa_kernels_gpu.py: B = 3 slots (slot
2 idle, pos = -1), smax = 192, a 12-page pool behind a non-identity block
table whose last entry per slot is -1. All four cache buffers (K codes, V
codes, K scales, V scales) are over-allocated by a guard tail and
pre-filled with the byte 0xCD, so "the right bytes were written, bit for
bit" and "nothing else was touched" are both checked.

Oracles:
  * append: engine/mx.py::quantize_mxfp8 on the fp16 source rows, every
    written code and scale byte compared bit for bit. The host codec and
    the device disagree on one thing only, the scale byte of an all-zero
    block (host 119, device 127; NOTES.md): cases (a) and (b) assert that
    no source block is all zero, case (c) expects the device's 127.
  * attention: the fp64 oracle on the DEQUANTISED K/V, atol = 1e-3,
    rtol = 0, no excluded elements. The bound is the one derived in
    tests/test_gqa_kernels_gpu.py: dequantisation is exact in fp32 (a
    4-bit significand times a power of two), |dequantised V| <= 1 (the
    block maximum quantises to at most 1.75 * 2^e <= amax), so what is
    left is fp32 accumulation, __expf and the fp16 rounding of an output
    in [-1, 1], as there.
"""
import functools

import numpy as np
import pytest
import torch

import trtlab_amd
from trtlab_amd.engine.mx import dequantize_mxfp8, quantize_mxfp8

pytestmark = pytest.mark.gpu

B, SMAX = 3, 192
NPAGES, MAXP = 12, 4
TABLE = np.array([[7, 2, 9, -1], [4, 11, 0, -1], [5, 1, 8, -1]], np.int32)
SENT = 0xCD
OUT_SENT = np.uint16(0xCDCD).view(np.int16)
GUARD = 4096
ATOL = 1e-3
HEADS = [(2, 2), (4, 2), (4, 1), (8, 1)]  # (Hq, Hkv)


@pytest.fixture(scope="module")
def C():
    return trtlab_amd.native()


def _uniform(seed, *shape):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(*shape, generator=g) * 2 - 1


def _sentinel(nbytes):
    return np.full(nbytes, SENT, np.uint8)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _paged_args(layout):
    if layout == "dense":
        return None, {}
    dt = _dev(TABLE)
    return dt, dict(table=dt.data_ptr(), max_pages=MAXP)


def _row_off(layout, b, h, t, H, D, smax=SMAX):
    """Element (= code byte) offset of row t of (slot b, cache head h) in
    a cache of H heads; None if the page is unmapped. The row's scale
    bytes start at this offset / 32."""
    if layout == "dense":
        return ((b * H + h) * smax + t) * D
    page = int(TABLE[b, t >> 6]) if (t >> 6) < MAXP else -1
    if page < 0:
        return None
    return ((page * 64 + (t & 63)) * H + h) * D


def _cache_elems(layout, H, D):
    return (B * H * SMAX if layout == "dense" else NPAGES * 64 * H) * D


def _quant_rows(x):
    """[..., D] fp16 tensor -> (codes u8 [..., D], scales u8 [..., D/32])."""
    D = x.shape[-1]
    codes, scales = quantize_mxfp8(x.float().reshape(-1, D).numpy())
    return (codes.reshape(*x.shape), scales.reshape(*x.shape[:-1], D // 32))


# ------------------------------------------------------------------ append
def _append_source(kind, Hq, Hkv, D, rows):
    """fp16 qkv [B*rows, (Hq+2Hkv)*D]. kind "uniform": [-1, 1]. "scaled":
    block j of kv head h of source row r times 2^((r + 3h + 5j) % 12 - 8),
    K and V alike, so the scale byte differs per block, head and row.
    "zero": uniform with the K row of the last kv head of every slot's
    first source row set to zero."""
    M = B * rows
    qkv = _uniform(17 * D + rows + Hq * 7 + Hkv, M, Hq + 2 * Hkv, D)
    if kind == "scaled":
        r = torch.arange(M)[:, None, None]
        h = torch.arange(Hkv)[None, :, None]
        j = torch.arange(D // 32)[None, None, :]
        f = torch.pow(2.0, ((r + 3 * h + 5 * j) % 12 - 8).float())
        f = f.repeat_interleave(32, dim=2)  # [M, Hkv, D]
        qkv[:, Hq:Hq + Hkv] *= f
        qkv[:, Hq + Hkv:] *= f
    qkv = qkv.half()
    if kind == "zero":
        qkv[::rows, Hq + Hkv - 1] = 0
    return qkv


def _run_append(C, layout, Hq, Hkv, D, rows, pos, kind="uniform"):
    """Returns {name: (got, expected, check mask)} for the four buffers."""
    qkv = _append_source(kind, Hq, Hkv, D, rows)
    ksrc, vsrc = qkv[:, Hq:Hq + Hkv], qkv[:, Hq + Hkv:]
    kzero = (ksrc.reshape(-1, 32) == 0).all(1)
    vzero = (vsrc.reshape(-1, 32) == 0).all(1)
    if kind == "zero":
        assert int(kzero.sum()) == B * (D // 32) and not vzero.any()
    else:  # the host codec's all-zero scale byte differs from the device's
        assert not kzero.any() and not vzero.any()
    kc, ks = _quant_rows(ksrc)
    vc, vs = _quant_rows(vsrc)
    ks = np.where(kzero.reshape(ks.shape).numpy(), 127, ks).astype(np.uint8)
    if kind == "zero":
        assert (kc[::rows, Hkv - 1] == 0).all()
        assert (ks[::rows, Hkv - 1] == 127).all()
    if kind == "scaled":  # the scale bytes really differ (6 exponents at
        # the smallest case: 3 source rows, 1 head, 2 blocks)
        assert len(np.unique(ks)) >= 4 and len(np.unique(vs)) >= 4

    elems = _cache_elems(layout, Hkv, D)
    S = D // 32
    exp = {"K": _sentinel(elems + GUARD), "V": _sentinel(elems + GUARD),
           "Ks": _sentinel(elems // 32 + GUARD),
           "Vs": _sentinel(elems // 32 + GUARD)}
    writers = np.zeros(elems // D, np.int32)  # per cache row
    for b in range(B):
        if pos is not None and pos[b] < 0:
            continue
        for q in range(rows):
            p = min((pos[b] if pos is not None else 0) + q, SMAX - 1)
            for h in range(Hkv):
                off = _row_off(layout, b, h, p, Hkv, D)
                if off is None:
                    continue
                r = b * rows + q
                exp["K"][off:off + D] = kc[r, h]
                exp["V"][off:off + D] = vc[r, h]
                so = off // 32
                exp["Ks"][so:so + S] = ks[r, h]
                exp["Vs"][so:so + S] = vs[r, h]
                writers[off // D] += 1
    dev = {n: _dev(_sentinel(len(e))) for n, e in exp.items()}
    dq = qkv.reshape(B * rows, -1).contiguous().cuda()
    dpos = _dev(np.asarray(pos, np.int32)) if pos is not None else None
    dt, kw = _paged_args(layout)
    torch.cuda.synchronize()
    C.ops.kv_append(dq.data_ptr(), dev["K"].data_ptr(), dev["V"].data_ptr(),
                    B, Hq, rows, SMAX,
                    pos=dpos.data_ptr() if dpos is not None else 0, D=D,
                    kv_heads=Hkv, kscale=dev["Ks"].data_ptr(),
                    vscale=dev["Vs"].data_ptr(), kv_format=1, **kw)
    once = writers <= 1
    code_ok = np.concatenate([np.repeat(once, D), np.ones(GUARD, bool)])
    scale_ok = np.concatenate([np.repeat(once, S), np.ones(GUARD, bool)])
    check = {"K": code_ok, "V": code_ok, "Ks": scale_ok, "Vs": scale_ok}
    return {n: (dev[n].cpu().numpy(), exp[n], check[n]) for n in exp}


def _assert_cache(res):
    for name, (got, exp, check) in res.items():
        bad = (got != exp) & check
        print(f"{name}: {int((exp != SENT).sum())} non-sentinel bytes "
              f"expected, {int(bad.sum())} mismatches")
        assert not bad.any(), (
            f"{name}: {int(bad.sum())} bytes differ, first at "
            f"{int(np.flatnonzero(bad)[0])}: got "
            f"{got[np.flatnonzero(bad)[0]]}, expected "
            f"{exp[np.flatnonzero(bad)[0]]}")


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("layout", ["dense", "paged"])
@pytest.mark.parametrize("heads", HEADS)
@pytest.mark.parametrize("rows,pos", [(1, [62, 127, -1]), (3, [62, 127, -1]),
                                      (70, None)])
@pytest.mark.parametrize("kind", ["uniform", "scaled", "zero"])
def test_kv_append_mx8(C, kind, rows, pos, heads, layout, D):
    """rows 1 and 3 at positions crossing a page boundary, and a prefill
    range from a null pos; no position is written twice. Every written
    code and scale byte equals the host codec's, everything else (idle
    slot, unmapped page, guard tail) is still the sentinel."""
    res = _run_append(C, layout, *heads, D, rows, pos, kind)
    assert all(check.all() for _, _, check in res.values())
    _assert_cache(res)


@pytest.mark.parametrize("heads", HEADS)
def test_kv_append_mx8_clamped(C, heads):
    """A chunk running past smax piles up on position smax-1 of slot 0:
    that row (every kv head, codes and scale bytes) is the only content
    not checked."""
    Hq, Hkv = heads
    D = 64
    res = _run_append(C, "dense", Hq, Hkv, D, 3, [SMAX - 2, 5, -1])
    rows_off = [_row_off("dense", 0, h, SMAX - 1, Hkv, D) for h in range(Hkv)]
    want_c = np.sort(np.concatenate([np.arange(D) + o for o in rows_off]))
    want_s = np.sort(np.concatenate(
        [np.arange(D // 32) + o // 32 for o in rows_off]))
    for name in ("K", "V"):
        assert np.array_equal(np.flatnonzero(~res[name][2]), want_c)
    for name in ("Ks", "Vs"):
        assert np.array_equal(np.flatnonzero(~res[name][2]), want_s)
    _assert_cache(res)


# --------------------------------------------------------------- attention
@functools.lru_cache(maxsize=None)
def _attn_inputs(Hq, Hkv, D):
    """Quantised logical K/V [B, Hkv, SMAX, D] (codes, scales, dequantised
    values) and a 3-row-per-slot grouped qkv. Position t, head h, block j
    is scaled by 2^-((t + 3h + 5j) % 6), so neighbouring blocks, heads and
    positions carry different scale bytes."""
    s = Hq * 1000 + Hkv * 100 + D
    t = torch.arange(SMAX)[None, None, :, None]
    h = torch.arange(Hkv)[None, :, None, None]
    j = torch.arange(D // 32)[None, None, None, :]
    f = torch.pow(2.0, -((t + 3 * h + 5 * j) % 6).float()) \
        .repeat_interleave(32, dim=3)
    out = []
    for seed in (1, 2):
        x = (_uniform(seed + s, B, Hkv, SMAX, D) * f).half()
        codes, scales = _quant_rows(x)
        deq = dequantize_mxfp8(codes.reshape(-1, D),
                               scales.reshape(-1, D // 32))
        assert np.abs(deq).max() <= 1.0
        out.append((codes, scales,
                    torch.from_numpy(deq.reshape(B, Hkv, SMAX, D))))
    qkv3 = _uniform(3 + s, B, 3, (Hq + 2 * Hkv) * D).half()
    return out[0], out[1], qkv3


def _fill_cache(layout, src, upto, D):
    """Sentinel buffer holding logical rows 0..upto[b]-1 of every head of
    src [B, H, SMAX, W] u8 (W = D for codes, D/32 for scale bytes)."""
    _, H, _, W = src.shape
    buf = _sentinel(_cache_elems(layout, H, D) * W // D + GUARD)
    for b in range(B):
        for t in range(upto[b]):
            for h in range(H):
                off = _row_off(layout, b, h, t, H, D) * W // D
                buf[off:off + W] = src[b, h, t]
    return buf


def _run_attention(C, layout, Hq, Hkv, D, rows, pos, qsel, mode="gqa"):
    """mode "gqa": kv_heads=Hkv. "mha": the replicated problem (codes and
    scales of every kv head copied across its query group, 3*Hq*D-wide
    qkv) through the MHA path. Returns the whole output allocation."""
    hid = Hq * D
    (kc, ks, _), (vc, vs, _), qkv3 = _attn_inputs(Hq, Hkv, D)
    qkv = qkv3[:, qsel].reshape(B * rows, -1)
    kw2 = dict(kv_heads=Hkv)
    if mode != "gqa":
        G = Hq // Hkv
        kc, ks, vc, vs = (np.repeat(a, G, axis=1) for a in (kc, ks, vc, vs))
        x = qkv.reshape(B * rows, Hq + 2 * Hkv, D)
        qkv = torch.cat([x[:, :Hq],
                         x[:, Hq:Hq + Hkv].repeat_interleave(G, 1),
                         x[:, Hq + Hkv:].repeat_interleave(G, 1)], 1) \
            .reshape(B * rows, 3 * Hq * D)
        kw2 = {}
    upto = [max(p + rows, 0) if p >= 0 else 0 for p in pos]
    bufs = [_dev(_fill_cache(layout, a, upto, D)) for a in (kc, vc, ks, vs)]
    dq = qkv.contiguous().cuda()
    out = _dev(np.full(B * rows * hid + GUARD, OUT_SENT, np.int16))
    dpos = _dev(np.asarray(pos, np.int32))
    dt, kw = _paged_args(layout)
    torch.cuda.synchronize()
    C.ops.decode_attention(dq.data_ptr(), bufs[0].data_ptr(),
                           bufs[1].data_ptr(), out.data_ptr(),
                           dpos.data_ptr(), B, Hq, rows, SMAX,
                           1.0 / float(np.sqrt(D)), D=D,
                           kscale=bufs[2].data_ptr(),
                           vscale=bufs[3].data_ptr(), kv_format=1, **kw,
                           **kw2)
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
    assert (raw[nb * rows * hid:] == OUT_SENT).all(), "guard tail written"
    for b in range(nb):
        if pos[b] < 0:
            assert (out[b] == OUT_SENT).all(), "idle slot's rows written"
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
def test_decode_attention_mx8(C, rows, heads, D):
    """n = 1 is the degenerate softmax; n = 128..130 spans three pages and
    leaves lanes with unequal key counts. Dense and paged against the
    oracle on the dequantised cache; paged == dense and GQA ==
    MHA-on-replicated-cache bit for bit."""
    Hq, Hkv = heads
    pos = [0, 127, -1]
    qsel = _QSEL[rows]
    (_, _, kd), (_, _, vd), qkv3 = _attn_inputs(Hq, Hkv, D)
    ref = _oracle(kd, vd, qkv3[:, qsel], Hq, Hkv, D, pos, rows)
    dense = _run_attention(C, "dense", Hq, Hkv, D, rows, pos, qsel)
    paged = _run_attention(C, "paged", Hq, Hkv, D, rows, pos, qsel)
    _check_oracle(dense, ref, B, rows, Hq * D, pos)
    _check_oracle(paged, ref, B, rows, Hq * D, pos)
    assert np.array_equal(dense, paged), "paged != dense"
    for layout, got in (("dense", dense), ("paged", paged)):
        mha = _run_attention(C, layout, Hq, Hkv, D, rows, pos, qsel, "mha")
        assert np.array_equal(got, mha), \
            f"{layout}: GQA differs from MHA on the replicated cache"


# ------------------------------------------------------------- error paths
@pytest.mark.parametrize("op", ["kv_append", "decode_attention"])
@pytest.mark.parametrize("case", ["no_scales", "one_scale", "unknown"])
def test_kv_format_errors(C, op, case):
    """kv_format=1 without both scale buffers, and an unknown kv_format,
    throw the named message before any launch."""
    buf = _dev(_sentinel(GUARD))
    dpos = _dev(np.full(B, -1, np.int32))
    torch.cuda.synchronize()
    p = buf.data_ptr()
    kw = {"no_scales": dict(kv_format=1),
          "one_scale": dict(kv_format=1, kscale=p),
          "unknown": dict(kv_format=7, kscale=p, vscale=p)}[case]
    msg = (f"{op}: unknown kv_format" if case == "unknown"
           else f"{op}: mxfp8 cache needs kscale and vscale")
    with pytest.raises(RuntimeError, match=msg):
        if op == "kv_append":
            C.ops.kv_append(p, p, p, B, 4, 1, SMAX, pos=dpos.data_ptr(),
                            D=64, kv_heads=2, **kw)
        else:
            C.ops.decode_attention(p, p, p, p, dpos.data_ptr(), B, 4, 1,
                                   SMAX, 0.125, D=64, kv_heads=2, **kw)
    torch.cuda.synchronize()
    assert (buf.cpu().numpy() == SENT).all()
