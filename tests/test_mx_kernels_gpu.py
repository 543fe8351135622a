"""MX (fp8-e4m3 / fp4-e2m1 + e8m0 block scales) kernels, pinned at the op
level: both GEMM tile sizes with row and column tails, every K-tile count
the 3-slot pipeline treats differently, the fp16 epilogues, the launcher
guards and the row quantizers.

Oracles run on the host in fp32. GEMM results are checked against the
matmul of the dequantized operands (rtol = atol = 1e-2 for fp32 output, as
test_kernels_gpu.test_gemm_mxfp8 does; the fp16 tolerance of that file's
`check` for fp16 output); quantizer codes and scales are bit-equal to numpy.
"""
import functools

import numpy as np
import pytest
import torch

import trtlab_amd
from trtlab_amd.engine import mx

pytestmark = pytest.mark.gpu

# M, N: the 128-tile kernel needs cdiv(M,128)*cdiv(N,128) >= 64. 1000x1016 is
# 8x8 tiles with a row tail of 104 and a column tail of 120 (a multiple of 8
# but not of 16: the last 16-wide fragment is half predicated). 72x40 takes
# the 64-tile kernel: 2x1 tiles, tails 8 and 40.
BIG = (1000, 1016)
SMALL = (72, 40)
KTILE = {"fp8": 128, "fp4": 256}  # logical k per staged LDS tile
PAD_ROWS = 16  # sentinel rows behind C
SENTINEL = {torch.float32: 0x7FC0BEEF, torch.float16: 0x7E5A}

QUANT = {"fp8": mx.quantize_mxfp8, "fp4": mx.quantize_mxfp4}
DEQUANT = {"fp8": mx.dequantize_mxfp8, "fp4": mx.dequantize_mxfp4}


@pytest.fixture(scope="module")
def C():
    return trtlab_amd.native()


def check(out, ref, rtol=2e-2, atol=2e-2, frac=1e-3):
    out = out.float().cpu()
    ref = ref.float().cpu()
    err = (out - ref).abs()
    tol = atol + rtol * ref.abs()
    bad = (err > tol).float().mean().item()
    assert bad <= frac, f"mismatch frac {bad}: max err {err.max()} vs {ref.abs().max()}"


@functools.lru_cache(maxsize=None)
def operands(fmt, M, N, K, spread=1.0):
    """Quantized A [M,K], B [N,K] on the device plus the host oracle
    dequant(A) @ dequant(B)^T. Row-varying magnitudes so the e8m0 scales
    differ; `spread` < 1 keeps the products inside fp16 range."""
    rng = np.random.RandomState(M + N + K)
    a32 = (rng.randn(M, K) * np.exp(spread * rng.randn(M, 1))).astype(np.float32)
    b32 = (rng.randn(N, K) * np.exp(spread * rng.randn(N, 1))).astype(np.float32)
    aq, asc = QUANT[fmt](a32)
    bq, bsc = QUANT[fmt](b32)
    ref = torch.from_numpy(DEQUANT[fmt](aq, asc)) @ \
        torch.from_numpy(DEQUANT[fmt](bq, bsc)).t()
    dev = tuple(torch.from_numpy(x).cuda() for x in (aq, bq, asc, bsc))
    return dev, ref


def run_gemm(C, fmt, M, N, K, dev, dtype=torch.float32, epi=0, scale=None,
             bias=None):
    """Run the op into a sentinel-filled [M + PAD_ROWS, N] buffer, assert the
    pad rows are untouched and all of [M, N] was written; returns [M, N]."""
    a, b, sa, sb = dev
    ibits = torch.int32 if dtype == torch.float32 else torch.int16
    raw = torch.full((M + PAD_ROWS, N), SENTINEL[dtype], dtype=ibits,
                     device="cuda")
    out = raw.view(dtype)
    assert torch.isnan(out).all()
    op = getattr(C.ops, "gemm_mx" + fmt)
    op(a.data_ptr(), b.data_ptr(), sa.data_ptr(), sb.data_ptr(),
       out.data_ptr(), M, N, K,
       out_dtype=2 if dtype == torch.float32 else 0, epi=epi,
       scale=scale.data_ptr() if scale is not None else 0,
       bias=bias.data_ptr() if bias is not None else 0)
    assert (raw[M:] == SENTINEL[dtype]).all(), "rows past M were written"
    assert not torch.isnan(out[:M]).any(), "an element of [M, N] was not written"
    return out[:M]


def gemm_cases():
    for fmt in ("fp8", "fp4"):
        # 1, 2, 3, 4 K-tiles: prologue only / no third stage / all three
        # slots / slot 0 reused
        for kt in (1, 2, 3, 4):
            yield fmt, *BIG, kt * KTILE[fmt]
        for kt in (1, 2, 3):
            yield fmt, *SMALL, kt * KTILE[fmt]


@pytest.mark.parametrize("fmt,M,N,K", list(gemm_cases()))
def test_gemm_mx_fp32(C, fmt, M, N, K):
    dev, ref = operands(fmt, M, N, K)
    out = run_gemm(C, fmt, M, N, K, dev)
    check(out, ref, rtol=1e-2, atol=1e-2)


def gelu_tanh(x):
    return 0.5 * x * (1.0 + torch.tanh(0.7978845608028654 * (x + 0.044715 * x ** 3)))


def epilogue_ref(acc, epi, scale, bias):
    v = acc
    if epi in (4, 5, 7):
        v = v * scale
    if epi != 0:
        v = v + bias
    if epi in (2, 5):
        v = torch.relu(v)
    if epi in (3, 7):
        v = gelu_tanh(v)
    return v


@pytest.mark.parametrize("M,N", [BIG, SMALL])
@pytest.mark.parametrize("fmt", ["fp8", "fp4"])
def test_gemm_mx_fp16_epilogues(C, fmt, M, N):
    K = 2 * KTILE[fmt]
    dev, ref = operands(fmt, M, N, K, spread=0.25)
    acc = run_gemm(C, fmt, M, N, K, dev)
    check(acc, ref, rtol=1e-2, atol=1e-2)
    assert acc.abs().max() < 6e4  # fp16 range, so the casts below are finite

    plain = run_gemm(C, fmt, M, N, K, dev, dtype=torch.float16)
    assert torch.equal(plain.view(torch.int16), acc.half().view(torch.int16))

    g = torch.Generator(device="cuda").manual_seed(N)
    scale = torch.rand(N, generator=g, device="cuda") + 0.5
    bias = torch.randn(N, generator=g, device="cuda") * 4.0
    for epi in (1, 2, 3, 4, 5, 7):
        out = run_gemm(C, fmt, M, N, K, dev, dtype=torch.float16, epi=epi,
                       scale=scale, bias=bias)
        check(out, epilogue_ref(acc, epi, scale, bias))


@pytest.mark.parametrize("fmt,K,msg", [
    ("fp8", 192, "gemm_mxfp8: K must be a multiple of 128"),
    ("fp4", 384, "gemm_mxfp4: K must be a multiple of 256"),
])
def test_gemm_mx_k_guard(C, fmt, K, msg):
    M = N = 64
    a = torch.zeros(M * K, dtype=torch.uint8, device="cuda")
    s = torch.full((M * K // 32,), 127, dtype=torch.uint8, device="cuda")
    out = torch.zeros(M, N, dtype=torch.float32, device="cuda")
    op = getattr(C.ops, "gemm_mx" + fmt)
    with pytest.raises(RuntimeError, match=msg):
        op(a.data_ptr(), a.data_ptr(), s.data_ptr(), s.data_ptr(),
           out.data_ptr(), M, N, K)


# ---- row quantizers ----
E2M1_MIDS = np.array([0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0], np.float32)


def quantizer_input(R, K):
    """fp16 rows with block-varying magnitudes and, in row 0 (and row 1 for
    the fp4 ties at another scale): an all-zero block, a block whose amax is
    exactly 2^2, and a block holding +-every e2m1 rounding midpoint after
    scaling (amax 6 -> shared exponent 0; the same block times 2^-3)."""
    rng = np.random.RandomState(R * K)
    nb = K // 32
    x = rng.randn(R, nb, 32) * np.exp(2.0 * rng.randn(R, nb, 1))
    x = np.clip(x, -6e4, 6e4).astype(np.float16)
    ties = np.zeros(32, np.float32)
    ties[:7], ties[7:14], ties[14] = E2M1_MIDS, -E2M1_MIDS, 6.0
    x[0, 0] = 0.0
    x[0, 1] = np.clip(x[0, 1], -3.0, 3.0)
    x[0, 1, 5] = -4.0
    x[0, 2] = ties
    x[1, 0] = ties * 0.125
    return x.reshape(R, K)


def block_exponent(x32, emax):
    """The device rule: floor(log2 amax) - emax clamped to +-127, and 0 for
    an all-zero block. Returns (e [R, K/32], amax)."""
    r, k = x32.shape
    amax = np.abs(x32.reshape(r, k // 32, 32)).max(axis=2)
    e = np.floor(np.log2(np.where(amax > 0, amax, 1.0))) - emax
    e = np.where(amax > 0, np.clip(e, -127, 127), 0.0)
    return e.astype(np.int32), amax


def quantize_mxfp4_oracle(x32):
    """The device rule: shared exponent as above, round to nearest on the
    e2m1 grid with exact midpoints going AWAY from zero."""
    r, k = x32.shape
    e, _ = block_exponent(x32, 2)
    q = (x32.reshape(r, k // 32, 32) * np.exp2(-e)[:, :, None].astype(np.float32))
    q = q.reshape(r, k)
    code = np.searchsorted(E2M1_MIDS, np.abs(q), side="right").astype(np.uint8)
    code = np.where(q < 0, code | 8, code).astype(np.uint8)
    return code[:, 0::2] | (code[:, 1::2] << 4), (e + 127).astype(np.uint8)


@pytest.mark.parametrize("R,K", [(3, 96), (9, 1024)])  # 9 / 288 blocks
@pytest.mark.parametrize("fmt", ["fp8", "fp4"])
def test_quantize_mx_rows(C, fmt, R, K):
    """Codes and scales bit-equal to the host oracle, every element.

    fp8 oracle: engine.mx.quantize_mxfp8 on the fp16-representable values,
    except the scale byte of an all-zero block: the device stores exponent 0
    (byte 127) there, the host codec 0 - emax (byte 119). The codes of such
    a block are zero under either scale. The difference predates this test
    and is recorded in NOTES.md, not fixed."""
    x = quantizer_input(R, K)
    x32 = x.astype(np.float32)
    e, amax = block_exponent(x32, 8 if fmt == "fp8" else 2)
    ref_scales = (e + 127).astype(np.uint8)
    if fmt == "fp8":
        ref_codes, host_scales = mx.quantize_mxfp8(x32)
        assert np.array_equal(host_scales[amax > 0], ref_scales[amax > 0])
        assert (amax == 0).sum() == 1 and host_scales[amax == 0] == 127 - 8
    else:
        ref_codes, oracle_scales = quantize_mxfp4_oracle(x32)
        assert np.array_equal(oracle_scales, ref_scales)

    xd = torch.from_numpy(x).cuda()
    codes = torch.full(ref_codes.shape, 0xA5, dtype=torch.uint8, device="cuda")
    scales = torch.full(ref_scales.shape, 0xA5, dtype=torch.uint8, device="cuda")
    getattr(C.ops, "quantize_mx" + fmt)(
        xd.data_ptr(), codes.data_ptr(), scales.data_ptr(), R, K)
    assert np.array_equal(scales.cpu().numpy(), ref_scales)
    assert np.array_equal(codes.cpu().numpy(), ref_codes)
