"""CPU definition of the MXFP8 KV cache: the row-size function and
run_reference(kv_format="mxfp8"), which round-trips every K/V head row
through the host MX codec before the attention scores."""
import numpy as np
import pytest


def test_kv_row_bytes():
    from trtlab_amd.engine.decode import kv_row_bytes

    assert kv_row_bytes(64, "fp16") == 128
    assert kv_row_bytes(128, "fp16") == 256
    assert kv_row_bytes(64, "mxfp8") == 66
    assert kv_row_bytes(128, "mxfp8") == 132
    assert kv_row_bytes(64) == 128  # fp16 is the default
    # 33/64 of fp16 for either head_dim
    for d in (64, 128):
        assert kv_row_bytes(d, "mxfp8") * 64 == kv_row_bytes(d, "fp16") * 33
    with pytest.raises(ValueError):
        kv_row_bytes(64, "fp4")


@pytest.fixture(scope="module")
def runs():
    from trtlab_amd.engine.planner import Planner
    from trtlab_amd.engine.reference import run_reference
    from trtlab_amd.models import build_llama

    g = build_llama(batch=2, seq=6, hidden=512, heads=4, kv_heads=2,
                    layers=2, vocab=5000)
    plan = Planner().compile(g)
    ids = np.random.RandomState(9).randint(1, 5000, 12).astype(np.int32)
    return (run_reference(plan, ids), run_reference(plan, ids, kv_format=None),
            run_reference(plan, ids, kv_format="mxfp8"), plan, ids)


def test_reference_default_unchanged(runs):
    plain, explicit, _, plan, ids = runs
    from trtlab_amd.engine.reference import run_reference

    assert np.array_equal(plain, explicit)
    assert np.array_equal(plain, run_reference(plan, ids, kv_format="fp16"))


def test_reference_mxfp8(runs):
    plain, _, mx, _, _ = runs
    assert mx.shape == plain.shape
    assert np.isfinite(mx).all()
    assert not np.array_equal(mx, plain)
    rel = np.abs(mx - plain).max() / np.abs(plain).max()
    print(f"mxfp8 vs fp32 K/V reference: rel {rel:.4f}")


def test_reference_rejects_unknown_format(runs):
    from trtlab_amd.engine.reference import run_reference

    with pytest.raises(ValueError):
        run_reference(runs[3], runs[4], kv_format="fp4")


def test_kv_roundtrip_is_row_codec():
    """The round trip is exactly quantize/dequantize of the fp16-rounded
    [*, D] rows, independent of the leading shape."""
    import torch

    from trtlab_amd.engine.mx import dequantize_mxfp8, quantize_mxfp8
    from trtlab_amd.engine.reference import _mx8_kv_roundtrip

    x = torch.randn(2, 3, 5, 64, generator=torch.Generator().manual_seed(1))
    got = _mx8_kv_roundtrip(x).numpy()
    rows = x.half().float().reshape(-1, 64).numpy()
    exp = dequantize_mxfp8(*quantize_mxfp8(rows)).reshape(2, 3, 5, 64)
    assert np.array_equal(got, exp)
