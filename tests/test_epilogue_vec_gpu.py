"""Vectorized conv/GEMM epilogues (channel-run MFMA output mapping).

Every kernel that stores through the shared channel-run epilogue is run on
shapes that hit both of its paths: the 16-byte vector path (whole channel
group inside N, aligned C / row pitch / residual) and the per-lane scalar
fallback (N % 8 != 0, odd ldc, pointers offset by one element).

Oracle: fp32 PyTorch on the same fp16 inputs, atol = rtol = 2e-2, and NO
excluded elements. fp16 rounding of the fp32 result is at most 2^-11
relative (bf16: 2^-8), well inside that tolerance at these K.
Scale and bias differ per channel (0.5 + n/N, 0.01*n) so a channel written
to the wrong column cannot pass. Outputs live in over-allocated buffers
pre-filled with a sentinel bit pattern; everything outside the logical
M x N (row padding when ldc > N, rows >= M, the element before an offset
pointer) must still hold the sentinel afterwards.

1-byte outputs add half a quantum of the output format to the tolerance,
since the oracle is not quantized: 0.5 for int8 (round to nearest integer),
2^-4 relative + 2^-10 absolute for fp8 e4m3 (3 mantissa bits: spacing 2^-3
relative, smallest subnormal 2^-9).
"""
import functools

import pytest
import torch

import trtlab_amd

pytestmark = pytest.mark.gpu

EPI_NONE, EPI_BIAS_RELU, EPI_SB_ADD_RELU = 0, 2, 6
ATOL = RTOL = 2e-2

# dtype code -> (torch dtype, raw integer view, sentinel bit pattern).
# fp8 sentinel 0x7F is NaN and the int8 one is -128 (never produced: the
# kernel clamps to +-127), so an unwritten logical element fails numerics.
_DT = {
    0: (torch.half, torch.int16, 0x7BCD),
    1: (torch.bfloat16, torch.int16, 0x7BCD),
    2: (torch.int8, torch.uint8, 0x80),
    3: (torch.float8_e4m3fn, torch.uint8, 0x7F),
}
_GUARD_ROWS = 64  # rows past M a 128-row tile could reach if unpredicated


@pytest.fixture(scope="module")
def C():
    return trtlab_amd.native()


def _chan_scale_bias(n):
    ar = torch.arange(n, dtype=torch.float32)
    return 0.5 + ar / n, ar * 0.01


def _sentinel_buf(dtype, elems):
    _, raw_dt, pat = _DT[dtype]
    return torch.full((elems,), pat, dtype=raw_dt, device="cuda")


def _logical_index(off, rows, ld, cols):
    r = torch.arange(rows).unsqueeze(1)
    c = torch.arange(cols).unsqueeze(0)
    return (off + r * ld + c).reshape(-1)


def _read_and_check_padding(buf, dtype, off, rows, ld, cols):
    """Logical [rows, cols] as fp32 on the CPU; asserts the rest of the
    buffer still holds the sentinel."""
    tdt, _, pat = _DT[dtype]
    raw = buf.cpu()
    idx = _logical_index(off, rows, ld, cols)
    outside = torch.ones(raw.numel(), dtype=torch.bool)
    outside[idx] = False
    touched = int((raw[outside] != raw.new_tensor(pat)).sum())
    assert touched == 0, f"{touched} elements outside the logical MxN written"
    return raw[idx].view(tdt).float().reshape(rows, cols)


def _assert_close(out, ref, extra_abs=0.0, extra_rel=0.0):
    err = (out - ref).abs()
    tol = ATOL + extra_abs + (RTOL + extra_rel) * ref.abs()
    ok = err <= tol  # NaN (unwritten fp8 sentinel) compares false
    print(f"max err {float(err[ok].max()) if ok.any() else float('nan'):.4g} "
          f"ref max {float(ref.abs().max()):.4g} bad {int((~ok).sum())}")
    assert bool(ok.all()), (
        f"{int((~ok).sum())} of {ok.numel()} elements out of tolerance, "
        f"first at {torch.nonzero(~ok)[0].tolist()}")


# ------------------------------------------------------------------ gemm_bt
@functools.lru_cache(maxsize=None)
def _gemm_inputs(dtype, M, N, K):
    """(a, b) on the device and the fp32 CPU product a @ b^T, computed once
    per shape and shared (read-only) by every case that uses the shape."""
    tdt = _DT[dtype][0]
    g = torch.Generator().manual_seed(1000 * dtype + M + 3 * N + 7 * K)
    if dtype == 2:
        a = torch.randint(-127, 128, (M, K), generator=g, dtype=torch.int8)
        b = torch.randint(-127, 128, (N, K), generator=g, dtype=torch.int8)
    else:
        a = torch.randn(M, K, generator=g).to(tdt)
        b = (torch.randn(N, K, generator=g) * 0.7 + 0.1).to(tdt)
    acc = a.float() @ b.float().t()
    res = torch.randn(M, N, generator=g)
    if dtype == 2:
        res = torch.randint(-100, 101, (M, N), generator=g, dtype=torch.int8)
    else:
        res = (res * 4.0).to(tdt)
    return a.cuda().contiguous(), b.cuda().contiguous(), acc, res


def _run_gemm(C, dtype, M, N, K, tile, epi, ldc=None, out_off=0, res_off=0,
              acc_scale=1.0, res_scale=1.0):
    ld = ldc or N
    a, b, acc, res = _gemm_inputs(dtype, M, N, K)
    scale, bias = _chan_scale_bias(N)
    scale = scale * acc_scale
    elems = out_off + (M + _GUARD_ROWS) * ld + 64
    out_buf = _sentinel_buf(dtype, elems)
    esz = out_buf.element_size()
    # residual shares ldc with C; zero-filled past the logical rows
    res_raw = torch.zeros(res_off + (M + _GUARD_ROWS) * ld + 64,
                          dtype=_DT[dtype][1])
    res_raw[_logical_index(res_off, M, ld, N)] = \
        res.contiguous().view(_DT[dtype][1]).reshape(-1)
    res_buf = res_raw.cuda()
    d_scale, d_bias = scale.cuda(), bias.cuda()
    torch.cuda.synchronize()
    C.ops.gemm_bt(dtype, a.data_ptr(), b.data_ptr(),
                  out_buf.data_ptr() + out_off * esz,
                  scale=d_scale.data_ptr() if epi == EPI_SB_ADD_RELU else 0,
                  bias=d_bias.data_ptr() if epi != EPI_NONE else 0,
                  residual=(res_buf.data_ptr() + res_off * esz
                            if epi == EPI_SB_ADD_RELU else 0),
                  M=M, N=N, K=K, epi=epi, tile=tile, res_scale=res_scale,
                  ldc=ld)
    ref = acc
    if epi == EPI_BIAS_RELU:
        ref = torch.relu(acc + bias)
    elif epi == EPI_SB_ADD_RELU:
        ref = torch.relu(acc * scale + bias + res.float() * res_scale)
    out = _read_and_check_padding(out_buf, dtype, out_off, M, ld, N)
    return out, ref


@pytest.mark.parametrize("epi", [EPI_NONE, EPI_BIAS_RELU, EPI_SB_ADD_RELU])
@pytest.mark.parametrize("tile", [1, 2, 3, 4])
def test_gemm_bt_base(C, tile, epi):
    """Partial row tile; the second 64-wide column tile (and the upper
    half of a 128-wide one) has only 8 valid channels."""
    out, ref = _run_gemm(C, 0, 70, 72, 128, tile, epi)
    _assert_close(out, ref)


@pytest.mark.parametrize("M,N,K,tile", [(70, 100, 64, 3), (33, 36, 64, 4)])
def test_gemm_bt_unaligned_n(C, M, N, K, tile):
    """N % 8 != 0: odd row pitch, every lane on the scalar fallback."""
    out, ref = _run_gemm(C, 0, M, N, K, tile, EPI_SB_ADD_RELU)
    _assert_close(out, ref)


def test_gemm_bt_padded_ldc(C):
    """ldc = 80 > N: aligned pitch, vector path; padding stays sentinel."""
    out, ref = _run_gemm(C, 0, 70, 72, 128, 2, EPI_SB_ADD_RELU, ldc=80)
    _assert_close(out, ref)


def test_gemm_bt_unaligned_ldc(C):
    out, ref = _run_gemm(C, 0, 70, 72, 128, 1, EPI_SB_ADD_RELU, ldc=73)
    _assert_close(out, ref)


def test_gemm_bt_offset_output(C):
    """C (2-byte aligned only) forces the fallback; the element in front of
    it must stay untouched."""
    out, ref = _run_gemm(C, 0, 70, 72, 128, 4, EPI_SB_ADD_RELU, out_off=1)
    _assert_close(out, ref)


def test_gemm_bt_offset_residual(C):
    out, ref = _run_gemm(C, 0, 70, 72, 128, 3, EPI_SB_ADD_RELU, res_off=1)
    _assert_close(out, ref)


def test_gemm_bt_bf16(C):
    out, ref = _run_gemm(C, 1, 70, 72, 128, 2, EPI_SB_ADD_RELU)
    _assert_close(out, ref)


# 1-byte outputs: tile 4 stores 8-byte vectors (ldc = 72 is 8-aligned),
# tile 1 stores 16-byte vectors and needs the 16-aligned pitch ldc = 80.
@pytest.mark.parametrize("tile,ldc", [(4, None), (1, 80)])
def test_gemm_bt_int8(C, tile, ldc):
    # |acc| ~ 6e4 at K=128; 5e-4 maps it into the int8 range
    out, ref = _run_gemm(C, 2, 70, 72, 128, tile, EPI_SB_ADD_RELU, ldc=ldc,
                         acc_scale=5e-4, res_scale=0.5)
    _assert_close(out, ref.clamp(-127, 127), extra_abs=0.5)


@pytest.mark.parametrize("tile,ldc", [(4, None), (1, 80)])
def test_gemm_bt_fp8(C, tile, ldc):
    out, ref = _run_gemm(C, 3, 70, 72, 128, tile, EPI_SB_ADD_RELU, ldc=ldc)
    _assert_close(out, ref.clamp(-448, 448), extra_abs=2.0 ** -10,
                  extra_rel=2.0 ** -4)


# ------------------------------------------------------------------- conv2d
def _pack_w(w):
    # [Cout, Cin, KH, KW] -> [Cout][KH*KW*Cin] (already a multiple of 64)
    cout, cin, kh, kw = w.shape
    return w.permute(0, 2, 3, 1).reshape(cout, kh * kw * cin).contiguous()


@pytest.mark.parametrize("shape", [
    # (Nb, H, W, Cin, Cout, k, pad)
    (1, 9, 9, 64, 72, 1, 0),     # small-K direct path
    (1, 9, 9, 128, 72, 1, 0),    # staged path, 8 valid channels in tile 2
    (1, 9, 9, 64, 64, 3, 1),
    (2, 7, 7, 512, 72, 3, 1),    # split-K (72 K-tiles, 4 tiles) + reduce
    (2, 7, 7, 512, 128, 3, 1),   # split-K + reduce
])
def test_conv2d_sb_add_relu(C, shape):
    nb, h, w_, cin, cout, k, pad = shape
    M = nb * h * w_
    g = torch.Generator().manual_seed(sum(shape))
    x = torch.randn(nb, h, w_, cin, generator=g).half()
    wt = (torch.randn(cout, cin, k, k, generator=g)
          * (2.0 / (k * k * cin) ** 0.5) + 0.01).half()
    res = torch.randn(M, cout, generator=g).half()
    scale, bias = _chan_scale_bias(cout)
    dx, dw, dres = x.cuda(), _pack_w(wt).cuda(), res.cuda()
    ds, db = scale.cuda(), bias.cuda()
    zero = torch.zeros(64, dtype=torch.half, device="cuda")
    out_buf = _sentinel_buf(0, (M + _GUARD_ROWS) * cout + 64)
    torch.cuda.synchronize()
    C.ops.conv2d(0, dx.data_ptr(), dw.data_ptr(), out_buf.data_ptr(),
                 scale=ds.data_ptr(), bias=db.data_ptr(),
                 residual=dres.data_ptr(), zero_page=zero.data_ptr(), Nb=nb,
                 H=h, W=w_, C=cin, Cout=cout, KH=k, KW=k, sh=1, sw=1, ph=pad,
                 pw=pad, epi=EPI_SB_ADD_RELU)
    y = torch.nn.functional.conv2d(x.float().permute(0, 3, 1, 2), wt.float(),
                                   padding=pad)
    y = y.permute(0, 2, 3, 1).reshape(M, cout)
    ref = torch.relu(y * scale + bias + res.float())
    out = _read_and_check_padding(out_buf, 0, 0, M, cout, cout)
    _assert_close(out, ref)


# ---------------------------------------------------------- bottleneck_tail
@pytest.mark.parametrize("nb,hw,cm,co", [
    (1, 9, 64, 256),     # M = 81, 32-row tiles
    (1, 9, 128, 256),
    (1, 23, 64, 256),    # M = 529, partial last tile
    (1, 128, 64, 64),    # M = 16384: the 64-row-tile variant (>= 256 tiles)
])
def test_bottleneck_tail(C, nb, hw, cm, co):
    """Fused 3x3+BN+ReLU -> 1x1+BN+residual+ReLU vs the fp32 two-conv
    reference with the intermediate rounded to fp16 (as the kernel keeps
    it in LDS)."""
    M = nb * hw * hw
    g = torch.Generator().manual_seed(nb + hw + cm + co)
    x = (torch.randn(nb, hw, hw, cm, generator=g) * 0.5).half()
    w1 = (torch.randn(cm, cm, 3, 3, generator=g) / (9 * cm) ** 0.5).half()
    w2 = (torch.randn(co, cm, generator=g) / cm ** 0.5 + 0.01).half()
    res = (torch.randn(M, co, generator=g) * 0.5).half()
    s1, b1 = _chan_scale_bias(cm)
    s2, b2 = _chan_scale_bias(co)
    dev = [t.cuda() for t in (x, _pack_w(w1), w2, res, s1, b1, s2, b2)]
    dx, dw1, dw2, dres, ds1, db1, ds2, db2 = dev
    zero = torch.zeros(64, dtype=torch.half, device="cuda")
    out_buf = _sentinel_buf(0, (M + _GUARD_ROWS) * co + 64)
    torch.cuda.synchronize()
    C.ops.bottleneck_tail(0, dx.data_ptr(), dw1.data_ptr(), dw2.data_ptr(),
                          out_buf.data_ptr(), ds1.data_ptr(), db1.data_ptr(),
                          ds2.data_ptr(), db2.data_ptr(), dres.data_ptr(),
                          zero.data_ptr(), Nb=nb, H=hw, W=hw, Cm=cm, Co=co)
    t = torch.nn.functional.conv2d(x.float().permute(0, 3, 1, 2), w1.float(),
                                   padding=1)
    t = t.permute(0, 2, 3, 1).reshape(M, cm)
    t = torch.relu(t * s1 + b1).half().float()
    ref = torch.relu((t @ w2.float().t()) * s2 + b2 + res.float())
    out = _read_and_check_padding(out_buf, 0, 0, M, co, co)
    _assert_close(out, ref)
