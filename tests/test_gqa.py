"""Native grouped-query attention (kv_heads), CPU side: IR shapes, the
fp32 reference, the safetensors loader's native_gqa mode, planner
descriptors and the plan / ONNX round-trips."""
import json
import os

import numpy as np
import pytest
import torch

from trtlab_amd.engine.ir import Graph
from trtlab_amd.engine.planner import K_ATTENTION, K_ROPE, Planner
from trtlab_amd.engine.reference import run_reference
from trtlab_amd.models import build_llama, build_llama_from_safetensors


def _rel(a, b):
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-6))


# ---------------------------------------------------------------- IR shapes
def test_ir_shapes_and_validation():
    g = Graph("gqa_ir")
    m = 8
    x = g.input((m, (4 + 2 * 2) * 128), name="qkv")
    r = g.rope(x, heads=4, seq=m, kv_heads=2)
    assert g.tensors[r].shape == (m, 8 * 128)
    a = g.attention(r, heads=4, seq=m, causal=True, kv_heads=2)
    assert g.tensors[a].shape == (m, 512)
    att = g.nodes[-1]
    assert att.attrs["head_dim"] == 128 and att.attrs["kv_heads"] == 2
    assert g.nodes[-2].attrs["kv_heads"] == 2
    with pytest.raises(AssertionError):
        g.attention(r, heads=4, seq=m, kv_heads=3)
    with pytest.raises(AssertionError):
        g.rope(x, heads=4, seq=m, kv_heads=3)

    g2 = Graph("mha_ir")
    y = g2.input((m, 3 * 512), name="qkv")
    y = g2.rope(y, heads=4, seq=m)
    g2.attention(y, heads=4, seq=m)
    assert "kv_heads" not in g2.nodes[-1].attrs
    assert "kv_heads" not in g2.nodes[-2].attrs
    assert g2.nodes[-1].attrs["head_dim"] == 128


# ------------------------------------------------------ reference equivalence
def _replicated_mha(g_gqa, heads, kvh, **kw):
    """MHA graph carrying g_gqa's weights with every kv head's k/v row
    block repeated across its query group."""
    g = build_llama(heads=heads, **kw)
    src = {n.name: n for n in g_gqa.nodes}
    for n in g.nodes:
        s = src[n.name]
        for key in ("weight", "gamma", "tok", "pos"):
            if key not in s.attrs or s.attrs[key] is None:
                continue
            val = s.attrs[key]
            if n.name.endswith("_qkv"):
                hd = val.shape[0] // (heads + 2 * kvh)
                blocks = val.reshape(heads + 2 * kvh, hd, -1)
                q, k, v = (blocks[:heads], blocks[heads:heads + kvh],
                           blocks[heads + kvh:])
                rep = heads // kvh
                val = np.concatenate(
                    [q, np.repeat(k, rep, axis=0), np.repeat(v, rep, axis=0)],
                    axis=0).reshape(3 * heads * hd, -1)
            n.attrs[key] = val
    return g


@pytest.mark.parametrize("kvh", [1, 2])
def test_reference_matches_replicated_mha(kvh):
    kw = dict(batch=1, seq=24, hidden=256, layers=2, vocab=300)
    g = build_llama(heads=4, kv_heads=kvh, **kw)
    gm = _replicated_mha(g, 4, kvh, **kw)
    p, pm = Planner().compile(g), Planner().compile(gm)
    ids = np.random.RandomState(3).randint(0, 300, 24).astype(np.int32)
    a, b = run_reference(p, ids), run_reference(pm, ids)
    assert a.shape == b.shape
    assert _rel(a, b) < 1e-5, _rel(a, b)


def test_build_llama_default_is_unchanged():
    """kv_heads=None draws the same random numbers into the same shapes
    as before; kv_heads=heads is the MHA shape too, spelled as GQA."""
    kw = dict(batch=1, seq=16, hidden=256, layers=1, heads=4, vocab=100)
    a, b = build_llama(**kw), build_llama(kv_heads=None, **kw)
    for na, nb in zip(a.nodes, b.nodes):
        assert na.name == nb.name and set(na.attrs) == set(nb.attrs)
        for k, v in na.attrs.items():
            if isinstance(v, np.ndarray):
                assert np.array_equal(v, nb.attrs[k])
            else:
                assert v == nb.attrs[k]
    nodes = {n.name: n for n in a.nodes}
    assert nodes["l0_qkv"].attrs["weight"].shape == (3 * 256, 256)
    assert "kv_heads" not in nodes["l0_att"].attrs


# ---------------------------------------------------------- checkpoint loader
H, LAYERS, HEADS, VOCAB, INTER = 256, 2, 4, 300, 448
EPS, THETA = 1e-6, 10000.0


def _mk_checkpoint(tmpdir, kvh):
    from safetensors.numpy import save_file

    rng = np.random.RandomState(7 + kvh)
    hd = H // HEADS
    kv_rows = kvh * hd

    def w(o, i):
        return (rng.randn(o, i) / np.sqrt(i)).astype(np.float32)

    st = {"model.embed_tokens.weight":
          (rng.randn(VOCAB, H) * 0.05).astype(np.float32),
          "model.norm.weight":
          rng.uniform(0.9, 1.1, H).astype(np.float32)}
    for li in range(LAYERS):
        p = f"model.layers.{li}."
        st[p + "input_layernorm.weight"] = \
            rng.uniform(0.9, 1.1, H).astype(np.float32)
        st[p + "post_attention_layernorm.weight"] = \
            rng.uniform(0.9, 1.1, H).astype(np.float32)
        for nm, shape in (("self_attn.q_proj", (H, H)),
                          ("self_attn.k_proj", (kv_rows, H)),
                          ("self_attn.v_proj", (kv_rows, H)),
                          ("self_attn.o_proj", (H, H)),
                          ("mlp.gate_proj", (INTER, H)),
                          ("mlp.up_proj", (INTER, H)),
                          ("mlp.down_proj", (H, INTER))):
            st[p + nm + ".weight"] = w(*shape)
    save_file(st, os.path.join(tmpdir, "model.safetensors"))
    with open(os.path.join(tmpdir, "config.json"), "w") as f:
        json.dump({"num_attention_heads": HEADS,
                   "num_key_value_heads": kvh,
                   "rope_theta": THETA, "rms_norm_eps": EPS}, f)
    return st


def _hf_forward(st, ids, seq, kvh):
    """Independent HF-semantics grouped-attention oracle (fp32 torch):
    query head h attends kv head h // (HEADS // kvh)."""
    hd = H // HEADS
    grp = HEADS // kvh

    def rms(x, g):
        v = x / torch.sqrt((x * x).mean(-1, keepdim=True) + EPS)
        return v * torch.from_numpy(g)

    def lin(x, wname):
        return x @ torch.from_numpy(st[wname]).t()

    def rope(x, pos):  # x [S, heads, hd] — HF rotate_half
        half = hd // 2
        inv = THETA ** (-torch.arange(half, dtype=torch.float64) * 2 / hd)
        ang = pos[:, None].double() * inv[None, :]
        cos = torch.cos(ang).float()[:, None, :]
        sin = torch.sin(ang).float()[:, None, :]
        x1, x2 = x[..., :half], x[..., half:]
        return torch.cat([x1 * cos - x2 * sin, x1 * sin + x2 * cos], -1)

    h = torch.from_numpy(st["model.embed_tokens.weight"])[ids]
    pos = torch.arange(seq)
    mask = torch.tril(torch.ones(seq, seq, dtype=torch.bool))
    for li in range(LAYERS):
        p = f"model.layers.{li}."
        x = rms(h, st[p + "input_layernorm.weight"])
        q = lin(x, p + "self_attn.q_proj.weight").view(seq, HEADS, hd)
        k = lin(x, p + "self_attn.k_proj.weight").view(seq, kvh, hd)
        v = lin(x, p + "self_attn.v_proj.weight").view(seq, kvh, hd)
        q, k = rope(q, pos), rope(k, pos)
        att = torch.zeros(seq, HEADS, hd)
        for hh in range(HEADS):
            sc = (q[:, hh] @ k[:, hh // grp].t()) / np.sqrt(hd)
            sc = sc.masked_fill(~mask, float("-inf"))
            att[:, hh] = torch.softmax(sc, -1) @ v[:, hh // grp]
        h = h + lin(att.reshape(seq, H), p + "self_attn.o_proj.weight")
        x = rms(h, st[p + "post_attention_layernorm.weight"])
        ff = torch.nn.functional.silu(lin(x, p + "mlp.gate_proj.weight")) * \
            lin(x, p + "mlp.up_proj.weight")
        h = h + lin(ff, p + "mlp.down_proj.weight")
    return rms(h, st["model.norm.weight"]).numpy()


@pytest.mark.parametrize("kvh", [1, 2])
def test_safetensors_native_gqa(tmp_path, kvh):
    st = _mk_checkpoint(str(tmp_path), kvh)
    seq, hd = 20, H // HEADS
    g = build_llama_from_safetensors(str(tmp_path), batch=1, seq=seq,
                                     native_gqa=True)
    nodes = {n.name: n for n in g.nodes}
    assert nodes["l0_qkv"].attrs["weight"].shape[0] == (HEADS + 2 * kvh) * hd
    assert nodes["l0_att"].attrs["kv_heads"] == kvh
    assert nodes["l0_rope"].attrs["kv_heads"] == kvh
    ids = np.random.RandomState(5).randint(0, VOCAB, seq).astype(np.int32)
    out = run_reference(Planner().compile(g), ids)
    ref = _hf_forward(st, torch.from_numpy(ids).long(), seq, kvh)
    assert _rel(out, ref) < 2e-3, _rel(out, ref)

    g0 = build_llama_from_safetensors(str(tmp_path), batch=1, seq=seq)
    n0 = {n.name: n for n in g0.nodes}
    assert n0["l0_qkv"].attrs["weight"].shape[0] == 3 * H
    assert "kv_heads" not in n0["l0_att"].attrs
    out0 = run_reference(Planner().compile(g0), ids)
    assert _rel(out0, ref) < 2e-3


# ------------------------------------------------------------------- planner
def _gqa_llama(kvh=2):
    return build_llama(batch=1, seq=24, hidden=256, heads=4, kv_heads=kvh,
                       layers=2, vocab=300)


def test_planner_descriptors():
    plan = Planner().compile(_gqa_llama(2))
    hd = 64
    ropes = [d for d in plan.ops if d["kind"] == K_ROPE]
    atts = [d for d in plan.ops if d["kind"] == K_ATTENTION]
    assert len(ropes) == 2 and len(atts) == 2
    for d in ropes + atts:
        assert d["NKV"] == 2 and d["NH"] == 4 and d["HD"] == hd
    by_name = dict(zip([o.name for o in plan.exec_ops], plan.ops))
    assert by_name["l0_qkv"]["N"] == (4 + 2 * 2) * hd

    mha = Planner().compile(build_llama(batch=1, seq=24, hidden=256, heads=4,
                                        layers=2, vocab=300))
    assert all("NKV" not in d for d in mha.ops)


def test_plan_io_roundtrip(tmp_path):
    from trtlab_amd.engine.plan_io import load_plan, save_plan

    plan = Planner().compile(_gqa_llama(2))
    pth = os.path.join(str(tmp_path), "gqa.npz")
    save_plan(plan, pth)
    plan2 = load_plan(pth)
    assert [d.get("NKV") for d in plan2.ops] == \
        [d.get("NKV") for d in plan.ops]
    ids = np.random.RandomState(1).randint(0, 300, 24).astype(np.int32)
    assert np.array_equal(run_reference(plan, ids), run_reference(plan2, ids))


def test_onnx_roundtrip():
    from trtlab_amd.engine.onnx_io import export_onnx, import_onnx

    g = _gqa_llama(1)
    g2 = import_onnx(export_onnx(g))
    for kind in ("attention", "rope"):
        got = [n.attrs.get("kv_heads") for n in g2.nodes if n.kind == kind]
        assert got == [1, 1], (kind, got)
    ids = np.random.RandomState(1).randint(0, 300, 24).astype(np.int32)
    a = run_reference(Planner().compile(g), ids)
    b = run_reference(Planner().compile(g2), ids)
    assert np.array_equal(a, b)

    # the attribute is absent from MHA exports
    mha = build_llama(batch=1, seq=24, hidden=256, heads=4, layers=1,
                      vocab=300)
    assert b"kv_heads" not in export_onnx(mha)
    assert b"kv_heads" in export_onnx(g)
