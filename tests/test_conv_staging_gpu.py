"""Conv A-tile staging: tap-uniform path vs the general per-lane path.

conv2d picks the tap-uniform staging (scalar (kh, kw, ci0) cursor, row
decomposition hoisted out of the K-loop) whenever C is a multiple of the
K-tile (64 elements for 2-byte formats, 128 for 1-byte ones); staging=1
forces the general path. Both stage the same bytes into the same LDS image,
so for every case the two outputs must be bit-identical (torch.equal on the
raw buffers, guard rows included), and each must match the fp32 PyTorch
conv on the same inputs at the tolerance tests/test_epilogue_vec_gpu.py
uses for the op: atol = rtol = 2e-2, plus half an output quantum for the
1-byte formats (0.5 for int8; 2^-4 relative + 2^-10 absolute for fp8 e4m3).
Cases with C % K-tile != 0 take the general path under both settings and
pin down that the host-side choice leaves them alone.

bottleneck_tail's GEMM1 always uses the tap-uniform staging; it must be
bit-equal to conv2d(3x3, staging=1) followed by conv2d(1x1 + residual).
"""
import functools

import pytest
import torch

import trtlab_amd

pytestmark = pytest.mark.gpu

EPI_SB_RELU, EPI_SB_ADD_RELU = 5, 6
ATOL = RTOL = 2e-2

# dtype code -> (torch dtype, raw integer view, sentinel, K-tile elements)
_DT = {
    0: (torch.half, torch.int16, 0x7BCD, 64),
    1: (torch.bfloat16, torch.int16, 0x7BCD, 64),
    2: (torch.int8, torch.uint8, 0x80, 128),
    3: (torch.float8_e4m3fn, torch.uint8, 0x7F, 128),
}
_GUARD_ROWS = 64


@pytest.fixture(scope="module")
def C():
    return trtlab_amd.native()


def _chan_scale_bias(n):
    ar = torch.arange(n, dtype=torch.float32)
    return 0.5 + ar / n, ar * 0.01


def _pack_w(w, kt):
    """[Cout, Cin, KH, KW] -> [Cout][KH*KW*Cin], K zero-padded to the tile."""
    cout, cin, kh, kw = w.shape
    raw = w.view(torch.uint8 if w.element_size() == 1 else torch.int16)
    flat = raw.permute(0, 2, 3, 1).reshape(cout, kh * kw * cin)
    k = flat.shape[1]
    kp = (k + kt - 1) // kt * kt
    if kp != k:  # all-zero bits are 0.0 / 0 in every format used here
        flat = torch.nn.functional.pad(flat, (0, kp - k))
    return flat.contiguous()


@functools.lru_cache(maxsize=None)
def _case(dtype, shape):
    """Device inputs and the fp32 CPU reference of relu(conv*scale + bias +
    res*res_scale), computed once per (dtype, shape) and shared read-only."""
    nb, h, w_, cin, cout, kh, kw, stride, ph, pw = shape
    tdt, raw_dt, _, kt = _DT[dtype]
    g = torch.Generator().manual_seed(1000 * dtype + sum(shape) + 7 * cin)
    fan = kh * kw * cin
    acc_scale, res_scale = 1.0, 1.0
    if dtype == 2:
        x = torch.randint(-64, 65, (nb, h, w_, cin), generator=g,
                          dtype=torch.int8)
        wt = torch.randint(-64, 65, (cout, cin, kh, kw), generator=g,
                           dtype=torch.int8)
        # |acc| ~ 37^2 * sqrt(fan): map ~2 sigma onto the int8 range
        acc_scale, res_scale = 60.0 / (1369.0 * fan ** 0.5), 0.5
    else:
        x = torch.randn(nb, h, w_, cin, generator=g).to(tdt)
        wt = (torch.randn(cout, cin, kh, kw, generator=g)
              * (2.0 / fan ** 0.5) + 0.01).to(tdt)
    y = torch.nn.functional.conv2d(x.float().permute(0, 3, 1, 2), wt.float(),
                                   stride=stride, padding=(ph, pw))
    oh, ow = y.shape[2], y.shape[3]
    M = nb * oh * ow
    y = y.permute(0, 2, 3, 1).reshape(M, cout)
    if dtype == 2:
        res = torch.randint(-100, 101, (M, cout), generator=g,
                            dtype=torch.int8)
    else:
        res = torch.randn(M, cout, generator=g).to(tdt)
    scale, bias = _chan_scale_bias(cout)
    scale = scale * acc_scale
    ref = torch.relu(y * scale + bias + res.float() * res_scale)
    if dtype == 2:
        ref = ref.clamp(-127, 127)
    elif dtype == 3:
        ref = ref.clamp(-448, 448)
    dev = dict(x=x.cuda().contiguous(), w=_pack_w(wt, kt).cuda(),
               res=res.cuda().contiguous(), scale=scale.cuda(),
               bias=bias.cuda(),
               zero=torch.zeros(128, dtype=torch.uint8, device="cuda"))
    torch.cuda.synchronize()
    return dev, ref, M, res_scale


def _run(C, dtype, shape, tile, staging):
    nb, h, w_, cin, cout, kh, kw, stride, ph, pw = shape
    tdt, raw_dt, pat, _ = _DT[dtype]
    dev, ref, M, res_scale = _case(dtype, shape)
    buf = torch.full(((M + _GUARD_ROWS) * cout,), pat, dtype=raw_dt,
                     device="cuda")
    torch.cuda.synchronize()
    C.ops.conv2d(dtype, dev["x"].data_ptr(), dev["w"].data_ptr(),
                 buf.data_ptr(), scale=dev["scale"].data_ptr(),
                 bias=dev["bias"].data_ptr(), residual=dev["res"].data_ptr(),
                 zero_page=dev["zero"].data_ptr(), Nb=nb, H=h, W=w_, C=cin,
                 Cout=cout, KH=kh, KW=kw, sh=stride, sw=stride, ph=ph, pw=pw,
                 epi=EPI_SB_ADD_RELU, tile=tile, res_scale=res_scale,
                 staging=staging)
    return buf.cpu()


def _assert_close(out, ref, extra_abs=0.0, extra_rel=0.0):
    err = (out - ref).abs()
    tol = ATOL + extra_abs + (RTOL + extra_rel) * ref.abs()
    ok = err <= tol  # NaN (an unwritten fp8 sentinel) compares false
    print(f"max err {float(err[ok].max()) if ok.any() else float('nan'):.4g} "
          f"ref max {float(ref.abs().max()):.4g} bad {int((~ok).sum())}")
    assert bool(ok.all()), (
        f"{int((~ok).sum())} of {ok.numel()} elements out of tolerance, "
        f"first at {torch.nonzero(~ok)[0].tolist()}")


_EXTRA = {0: (0.0, 0.0), 1: (0.0, 0.0), 2: (0.5, 0.0),
          3: (2.0 ** -10, 2.0 ** -4)}


def _check(C, dtype, shape, tile=0):
    tdt, _, pat, _ = _DT[dtype]
    cout = shape[4]
    auto = _run(C, dtype, shape, tile, staging=0)
    general = _run(C, dtype, shape, tile, staging=1)
    assert torch.equal(auto, general), (
        f"{int((auto != general).sum())} elements differ between staging=0 "
        f"and staging=1")
    _, ref, M, _ = _case(dtype, shape)
    guard = auto[M * cout:]
    assert bool((guard == guard.new_tensor(pat)).all()), "rows >= M written"
    out = auto[:M * cout].view(tdt).float().reshape(M, cout)
    ea, er = _EXTRA[dtype]
    _assert_close(out, ref, extra_abs=ea, extra_rel=er)


# shapes: (Nb, H, W, C, Cout, KH, KW, stride, ph, pw)
@pytest.mark.parametrize("tile", [1, 2, 3, 4])
def test_partial_tile_all_borders(C, tile):
    """M = 98: partial row tile and the m >= M clamp, all four borders;
    tile codes 1-2 stage 4 chunks per thread (BM = 128), 3-4 stage 2."""
    _check(C, 0, (2, 7, 7, 64, 64, 3, 3, 1, 1, 1), tile=tile)


@pytest.mark.parametrize("shape", [
    (1, 9, 9, 128, 64, 3, 3, 1, 1, 1),    # two K-tiles per tap: ci0 wraps
    (2, 8, 8, 64, 128, 3, 3, 2, 1, 1),    # stride 2 with padding
    (1, 9, 9, 192, 72, 3, 3, 1, 1, 1),    # C % 64 == 0, not a power of two;
                                          # Cout = 72: scalar epilogue lanes
    (1, 6, 10, 64, 64, 3, 1, 1, 1, 0),    # KH != KW, H != W: kh/kw swap
    (1, 5, 5, 64, 64, 5, 5, 1, 2, 2),     # most taps out of the image
    (2, 9, 9, 128, 64, 1, 1, 2, 0, 0),    # strided pointwise
    (1, 9, 9, 128, 72, 1, 1, 1, 0, 0),    # pointwise, staged (two K-tiles)
    (1, 9, 9, 256, 64, 1, 1, 1, 0, 0),    # four tiles: deep-pipe prologue
                                          # plus steady state
    (2, 7, 7, 512, 128, 3, 3, 1, 1, 1),   # split-K, ktper = 9: slices start
                                          # in mid-tap
])
def test_tap_uniform_fp16(C, shape):
    _check(C, 0, shape)


@pytest.mark.parametrize("shape", [
    (1, 9, 9, 72, 64, 3, 3, 1, 1, 1),     # C % 64 != 0: zero-padded K-tile
    (1, 18, 18, 8, 64, 7, 7, 2, 3, 3),    # stem-like
])
def test_general_path_kept_fp16(C, shape):
    _check(C, 0, shape)


def test_tap_uniform_bf16(C):
    _check(C, 1, (1, 9, 9, 128, 64, 3, 3, 1, 1, 1))


@pytest.mark.parametrize("dtype", [2, 3])
@pytest.mark.parametrize("cin", [128, 64])
def test_one_byte_formats(C, dtype, cin):
    """K-tile = 128 elements: C = 128 takes the tap-uniform path, C = 64
    (half a K-tile per tap, zero-padded K tail) stays on the general one."""
    _check(C, dtype, (1, 9, 9, cin, 64, 3, 3, 1, 1, 1))


# ---------------------------------------------------------- bottleneck_tail
@pytest.mark.parametrize("nb,hw,cm,co", [
    (1, 9, 64, 256),     # M = 81, 32-row tiles
    (1, 9, 128, 256),    # two K-tiles per tap, two GEMM1 column chunks
    (1, 128, 64, 64),    # M = 16384: the 64-row-tile variant
])
def test_bottleneck_tail_matches_general_convs(C, nb, hw, cm, co):
    M = nb * hw * hw
    g = torch.Generator().manual_seed(nb + hw + cm + co)
    x = (torch.randn(nb, hw, hw, cm, generator=g) * 0.5).half()
    w1 = (torch.randn(cm, cm, 3, 3, generator=g) / (9 * cm) ** 0.5).half()
    w2 = (torch.randn(co, cm, generator=g) / cm ** 0.5 + 0.01).half()
    res = (torch.randn(M, co, generator=g) * 0.5).half()
    s1, b1 = _chan_scale_bias(cm)
    s2, b2 = _chan_scale_bias(co)
    dev = [t.cuda() for t in (x, _pack_w(w1, 64), w2, res, s1, b1, s2, b2)]
    dx, dw1, dw2, dres, ds1, db1, ds2, db2 = dev
    zero = torch.zeros(64, dtype=torch.half, device="cuda")
    fused = torch.full((M, co), float("nan"), dtype=torch.half, device="cuda")
    mid = torch.full((M, cm), float("nan"), dtype=torch.half, device="cuda")
    two = torch.full((M, co), float("nan"), dtype=torch.half, device="cuda")
    torch.cuda.synchronize()
    C.ops.bottleneck_tail(0, dx.data_ptr(), dw1.data_ptr(), dw2.data_ptr(),
                          fused.data_ptr(), ds1.data_ptr(), db1.data_ptr(),
                          ds2.data_ptr(), db2.data_ptr(), dres.data_ptr(),
                          zero.data_ptr(), Nb=nb, H=hw, W=hw, Cm=cm, Co=co)
    C.ops.conv2d(0, dx.data_ptr(), dw1.data_ptr(), mid.data_ptr(),
                 scale=ds1.data_ptr(), bias=db1.data_ptr(),
                 zero_page=zero.data_ptr(), Nb=nb, H=hw, W=hw, C=cm, Cout=cm,
                 KH=3, KW=3, sh=1, sw=1, ph=1, pw=1, epi=EPI_SB_RELU,
                 staging=1)
    C.ops.conv2d(0, mid.data_ptr(), dw2.data_ptr(), two.data_ptr(),
                 scale=ds2.data_ptr(), bias=db2.data_ptr(),
                 residual=dres.data_ptr(), zero_page=zero.data_ptr(), Nb=nb,
                 H=hw, W=hw, C=cm, Cout=co, KH=1, KW=1, epi=EPI_SB_ADD_RELU)
    fused, two = fused.cpu(), two.cpu()
    assert not bool(torch.isnan(two).any())
    assert torch.equal(fused.view(torch.int16), two.view(torch.int16)), (
        f"{int((fused != two).sum())} of {fused.numel()} elements differ")
