"""Incremental (KV-cache) decoding for GPT-2- and LLaMA-family models.

Beyond-reference capability (the CUDA reference served static TensorRT
engines only): a `DecodeSession` holds per-layer K/V caches resident in
HBM and replays ONE hipGraph per generated token. All position dependence
flows through a device-side counter (csrc/kernels/decode.hip), so the
captured graph needs no re-instantiation between steps.

The transformer forward is written once, in `DecodeSession._forward`:

    norm1 -> [per layer: qkv gemm -> rope (LLaMA) -> kv_append +
    attention -> proj gemm -> +res, norm2 -> MLP -> +res, next norm1 |
    final norm]

recorded for a buffer set and one of three pass kinds: "step" (one row
per slot at the device position), "chunk" (K rows per slot, speculative
verification) and "prefill" (the whole padded prompt: append only, then
full-sequence causal attention). The GPT-2 / LLaMA difference (LayerNorm
+ biased GEMMs + GELU vs RMSNorm + RoPE + SwiGLU) lives in that one
function; the embedding in front and the lm head / argmax / advance_pos
behind it belong to the pass (`_enqueue`, `_enqueue_chunk`, `prefill`).
`_enqueue_fused` is the separate experimental fused-kernel step.

Caveat: the raw-op GEMMs share the lazily-grown module-level scratch
buffer (csrc/ext.cpp test_scratch); the captured graph bakes its address,
so other raw-op users must not force a regrow while a session is live
(engine-managed contexts are unaffected).

Weights come from a `build_gpt2(embeddings=True)` or `build_llama()` IR
graph (the same random-init builders the full-sequence engine uses, so
prefill/decode can be cross-checked). The recipe is detected from the
node names: `l0_rms1` present -> LLaMA (RMSNorm + RoPE + SwiGLU, no
biases; RoPE reads the device position counter, so the captured decode
graph stays position-free); otherwise GPT-2 (LayerNorm + learned pos
emb + GELU). prefill()/step()/verify_chunk() and the paged KV pool work
for both.

Grouped-query LLaMA graphs (`build_llama(kv_heads=...)`, attention nodes
carrying `kv_heads`) run natively: the qkv projection is
(heads + 2*kv_heads)*head_dim wide, the dense caches are
[B][kv_heads][smax][head_dim] and paged pools hold kv_heads heads per
position, so KV memory is heads/kv_heads x smaller than for MHA.

`kv_dtype="mxfp8"` (sessions and pools) stores K/V as MXFP8: e4m3 code
bytes in caches of the fp16 shape plus one e8m0 scale byte per 32
elements in separate `kscale` / `vscale` buffers — 33/64 of the fp16
bytes for any model, no calibration. kv_append quantises, the decode
attention dequantises in registers (csrc/kernels/decode.hip, element
format policy); `_kv()` is the only place that knows.
"""
from __future__ import annotations

from typing import Dict, List, Optional

import numpy as np

KV_DTYPES = ("fp16", "mxfp8")
_MX_BLOCK = 32  # elements per e8m0 scale byte


def kv_row_bytes(head_dim: int, kv_dtype: str = "fp16") -> int:
    """Bytes one (slot, kv head, position) row of K (or of V) occupies:
    fp16 2*head_dim; mxfp8 head_dim code bytes + head_dim/32 scale bytes."""
    if kv_dtype == "fp16":
        return 2 * head_dim
    if kv_dtype == "mxfp8":
        if head_dim % _MX_BLOCK:
            raise ValueError("mxfp8 KV rows need head_dim % 32 == 0")
        return head_dim + head_dim // _MX_BLOCK
    raise ValueError(f"unknown kv_dtype {kv_dtype!r} (fp16 | mxfp8)")



class PagedKVPool:
    """vLLM-style paged KV memory: ONE fixed physical pool per layer,
    shared by every slot, mapped through a per-slot device block table.
    Pages hold 64 positions x heads x head_dim, where `heads` is the
    number of KV heads (= query heads for MHA, fewer for grouped-query
    models); a page id is valid across all layers (each layer has its
    own K/V pools, ids allocated in lockstep), so one table serves the
    whole stack. Host-side free list; idle/reset slots return their
    pages — parked sequences hold ZERO cache memory (the paged payoff vs
    the dense [B][heads][smax][head_dim] layout).
    """

    def __init__(self, layers: int, heads: int, batch: int,
                 num_pages: int, max_pages_per_slot: int,
                 device: int = 0, head_dim: int = 64,
                 kv_dtype: str = "fp16"):
        """kv_dtype="mxfp8": the pools hold e4m3 bytes (same shape, u8)
        and `kscales` / `vscales` hold the per-32-element e8m0 bytes,
        [page][64][heads][head_dim/32] u8 per layer."""
        import torch

        from trtlab_amd import native

        kv_row_bytes(head_dim, kv_dtype)  # validates kv_dtype
        self._C = native()
        self._torch = torch
        torch.cuda.set_device(device)
        self.layers = layers
        self.heads = heads
        self.batch = batch
        self.num_pages = num_pages
        self.max_pages = max_pages_per_slot
        self.head_dim = head_dim
        self.kv_dtype = kv_dtype
        mx = kv_dtype == "mxfp8"
        self.kpools = [torch.zeros(num_pages, 64, heads, head_dim,
                                   dtype=torch.uint8 if mx else torch.half,
                                   device="cuda")
                       for _ in range(layers)]
        self.vpools = [torch.zeros_like(k) for k in self.kpools]
        self.kscales = [torch.zeros(num_pages, 64, heads,
                                    head_dim // _MX_BLOCK,
                                    dtype=torch.uint8, device="cuda")
                        for _ in range(layers)] if mx else None
        self.vscales = ([torch.zeros_like(k) for k in self.kscales]
                        if mx else None)
        self.table = torch.full((batch, max_pages_per_slot), -1,
                                dtype=torch.int32, device="cuda")
        self._table_host = np.full((batch, max_pages_per_slot), -1,
                                   np.int32)
        self._free = list(range(num_pages - 1, -1, -1))

    @property
    def pages_free(self) -> int:
        return len(self._free)

    def ensure(self, b: int, logical_idx: int) -> None:
        """Map slot b's logical page if unmapped (called by the session
        right before a step that will write position logical_idx*64+...)."""
        if logical_idx >= self.max_pages:
            raise RuntimeError(
                f"slot {b}: logical page {logical_idx} >= max_pages")
        if self._table_host[b, logical_idx] >= 0:
            return
        if not self._free:
            raise MemoryError(
                "PagedKVPool exhausted (all pages mapped) — free a slot")
        pid = self._free.pop()
        self._table_host[b, logical_idx] = pid
        ent = np.array([pid], np.int32)
        self._C.memory.memcpy_h2d(
            self.table.data_ptr() + (b * self.max_pages + logical_idx) * 4,
            ent, 4)

    def free_slot(self, b: int) -> int:
        """Return slot b's pages to the free list; returns count freed."""
        n = 0
        for i in range(self.max_pages):
            pid = int(self._table_host[b, i])
            if pid >= 0:
                self._free.append(pid)
                self._table_host[b, i] = -1
                n += 1
        row = np.full(self.max_pages, -1, np.int32)
        self._C.memory.memcpy_h2d(
            self.table.data_ptr() + b * self.max_pages * 4, row,
            row.nbytes)
        return n


class DecodeSession:
    """One generation session: fixed batch, growing position."""

    def __init__(self, graph, batch: int, smax: int = 1024, device: int = 0,
                 capture: bool = True, lm_head: bool = False,
                 fused: bool = False, paged=None, kv_dtype: str = "fp16"):
        """kv_dtype: "fp16" (default) or "mxfp8" — K/V cached as e4m3
        bytes plus per-32-element e8m0 scales (33/64 of the fp16 bytes;
        see kv_row_bytes / kv_cache_bytes). A PagedKVPool passed as
        `paged` must have been built with the same kv_dtype.

        fused=True (needs batch <= 64): EXPERIMENTAL horizontal kernel
        fusion for the latency-bound step — LN / residual-add / embed
        prologues and KV-scatter / GeLU epilogues fold into the small-M
        GEMMs (csrc decode_gemm_fused), cutting ~8 kernels/layer to 5.
        MEASURED on MI355X (profiles/README r2): the fused GEMMs lose
        split-K + the deep staging pipeline and only fill cdiv(N,64)
        workgroups, so the step is currently ~2x SLOWER than the unfused
        autotuned path (0.86 -> 1.63 ms b8) despite 40% fewer kernels —
        default OFF; numerics are verified (test_fused_decode_matches_
        unfused). Making the fused GEMM pipeline-deep is the round-3
        follow-up. The residual stream ping-pongs between two buffers
        (the fused ADD_LN writes the NEW stream while other blocks still
        read the old)."""
        import torch

        from trtlab_amd import native
        from trtlab_amd.engine.planner import (EPI_BIAS, EPI_BIAS_GELU,
                                               EPI_NONE)

        if kv_dtype not in KV_DTYPES:
            raise ValueError(f"unknown kv_dtype {kv_dtype!r} (fp16 | mxfp8)")
        if fused and kv_dtype != "fp16":
            raise ValueError("fused decode supports the fp16 KV cache only")
        self.kv_dtype = kv_dtype
        self._kv_format = KV_DTYPES.index(kv_dtype)  # the kernels' code
        self._C = native()
        self._torch = torch
        torch.cuda.set_device(device)
        self.batch = batch
        self.smax = smax
        self.capture = capture
        self._epi_bias = EPI_BIAS
        self._epi_gelu = EPI_BIAS_GELU
        self._epi_none = EPI_NONE

        # ---- pull weights out of the IR graph by node kind/name ----
        # Two layer recipes share the session plumbing (KV caches, paged
        # pool, graph capture, position counters, spec-decode chunks):
        #   gpt2  — LayerNorm + learned pos emb + GELU MLP (l{i}_ln1 ...)
        #   llama — RMSNorm + RoPE + SwiGLU, no biases   (l{i}_rms1 ...)
        nodes = {n.name: n for n in graph.nodes}
        self.arch = "llama" if "l0_rms1" in nodes else "gpt2"
        emb = next(n for n in graph.nodes if n.kind == "embedding")
        self.hidden = emb.attrs["tok"].shape[1]
        self.vocab = emb.attrs["tok"].shape[0]
        assert emb.attrs["pos"].shape[0] >= 1

        def dev16(a):
            return torch.from_numpy(np.ascontiguousarray(a, np.float32)) \
                .half().cuda()

        def dev32(a):
            return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()

        self.tok = dev16(emb.attrs["tok"])
        self.posemb = dev16(emb.attrs["pos"])
        if self.posemb.shape[0] < smax:
            self.smax = smax = int(self.posemb.shape[0])

        self.layers: List[Dict] = []
        li = 0
        while f"l{li}_qkv" in nodes:
            att = nodes[f"l{li}_att"]
            self.heads = att.attrs["heads"]
            # grouped-query: kv_heads < heads narrows the qkv row to
            # (heads + 2*kv_heads)*hd and the caches to kv_heads
            self.kv_heads = att.attrs.get("kv_heads") or self.heads
            self.hd = att.attrs.get("head_dim",
                                    self.hidden // self.heads)
            if self.hd not in (64, 128):
                raise ValueError("decode: head_dim must be 64 or 128")
            lay = {}
            if self.arch == "llama":
                self.rms_eps = float(
                    nodes[f"l{li}_rms1"].attrs.get("eps", 1e-5))
                lay["rms1_g"] = dev32(nodes[f"l{li}_rms1"].attrs["gamma"])
                lay["rms2_g"] = dev32(nodes[f"l{li}_rms2"].attrs["gamma"])
                self.theta = float(
                    nodes[f"l{li}_rope"].attrs.get("theta", 10000.0))
                for key in ("qkv", "proj", "gate", "up", "down"):
                    lay[key + "_w"] = dev16(nodes[f"l{li}_{key}"]
                                            .attrs["weight"])
            else:
                for key, nm in (("ln1", f"l{li}_ln1"), ("ln2", f"l{li}_ln2")):
                    lay[key + "_g"] = dev32(nodes[nm].attrs["gamma"])
                    lay[key + "_b"] = dev32(nodes[nm].attrs["beta"])
                for key in ("qkv", "proj", "ff1", "ff2"):
                    n = nodes[f"l{li}_{key}"]
                    lay[key + "_w"] = dev16(n.attrs["weight"])
                    lay[key + "_b"] = dev32(n.attrs["bias"])
            mx = kv_dtype == "mxfp8"
            lay["kcache"] = torch.zeros(
                batch, self.kv_heads, smax, self.hd,
                dtype=torch.uint8 if mx else torch.half, device="cuda")
            lay["vcache"] = torch.zeros_like(lay["kcache"])
            # mxfp8: one e8m0 byte per 32 elements, beside the codes
            lay["kscale"] = torch.zeros(
                batch, self.kv_heads, smax, self.hd // _MX_BLOCK,
                dtype=torch.uint8, device="cuda") if mx else None
            lay["vscale"] = (torch.zeros_like(lay["kscale"]) if mx
                             else None)
            self.layers.append(lay)
            li += 1
        self.n_layers = li
        if self.arch == "llama":
            if self.hidden > 2048:
                raise ValueError("llama decode: hidden > 2048 (rmsnorm "
                                 "kernel row limit)")
            self.inter = self.layers[0]["gate_w"].shape[0]
            self.lnf_g = dev32(nodes["rms_f"].attrs["gamma"])
            self.lnf_b = None
        else:
            self.inter = self.layers[0]["ff1_w"].shape[0]
            gf = nodes["ln_f"]
            self.lnf_g = dev32(gf.attrs["gamma"])
            self.lnf_b = dev32(gf.attrs["beta"])
        self.lm_head = lm_head  # logits = h @ tok^T (weight tying)

        B, Hd = batch, self.hidden
        # fused qkv row width; att rows are heads*hd (== hidden here)
        self.qkv_w = (self.heads + 2 * self.kv_heads) * self.hd
        self._nkv = self.kv_heads if self.kv_heads != self.heads else 0
        self.ids = torch.zeros(B, dtype=torch.int32, device="cuda")
        self.pos = torch.zeros(B, dtype=torch.int32, device="cuda")
        self._slot_steps = np.zeros(B, np.int64)
        self._active = np.ones(B, bool)  # host mirror of pos[b] >= 0
        self.h = torch.zeros(B, Hd, dtype=torch.half, device="cuda")
        self.x = torch.zeros(B, Hd, dtype=torch.half, device="cuda")
        self.qkv = torch.zeros(B, self.qkv_w, dtype=torch.half,
                               device="cuda")
        self.att = torch.zeros(B, Hd, dtype=torch.half, device="cuda")
        self.x2 = torch.zeros(B, Hd, dtype=torch.half, device="cuda")
        self.ff = torch.zeros(B, self.inter, dtype=torch.half, device="cuda")
        # SwiGLU needs gate AND up live at once (silu(gate) * up)
        self.ff2 = (torch.zeros(B, self.inter, dtype=torch.half,
                                device="cuda")
                    if self.arch == "llama" else None)
        self.out = torch.zeros(B, Hd, dtype=torch.half, device="cuda")
        self.logits = (torch.zeros(B, self.vocab, dtype=torch.half,
                                   device="cuda") if lm_head else None)
        # device-side greedy head: argmax ids land here every step (the
        # argmax kernel is captured in the step graph; step(return_ids=
        # True) then moves B ints instead of B*vocab logits over PCIe)
        self.gids = (torch.zeros(B, dtype=torch.int32, device="cuda")
                     if lm_head else None)
        self.supports_ids = lm_head
        # sample_tokens(..., top_k, top_p): device-side top-k / nucleus
        self.supports_truncation = lm_head
        self.h2 = torch.zeros(B, Hd, dtype=torch.half, device="cuda")
        # paged KV mode: paged = a PagedKVPool (shared with other
        # sessions) or True (private pool sized for smax). The dense
        # per-layer caches above are then released — slots draw pages on
        # demand and return them on idle/reset.
        self.kv_pool = None
        if paged:
            mp = (smax + 63) // 64
            self.kv_pool = paged if isinstance(paged, PagedKVPool) else \
                PagedKVPool(self.n_layers, self.kv_heads, B,
                            num_pages=B * mp, max_pages_per_slot=mp,
                            device=device, head_dim=self.hd,
                            kv_dtype=kv_dtype)
            if self.kv_pool.layers != self.n_layers or \
                    self.kv_pool.heads != self.kv_heads or \
                    self.kv_pool.head_dim != self.hd:
                raise ValueError("pool layer/head mismatch")
            if self.kv_pool.kv_dtype != kv_dtype:
                raise ValueError(
                    f"pool kv_dtype {self.kv_pool.kv_dtype!r} != session "
                    f"kv_dtype {kv_dtype!r}")
            for lay in self.layers:  # release the dense caches
                lay["kcache"] = None
                lay["vcache"] = None
                lay["kscale"] = None
                lay["vscale"] = None
        self.fused = bool(fused)
        if self.fused and self._nkv:
            raise ValueError("fused decode does not support grouped-query "
                             "attention (kv_heads < heads)")
        if self.fused and self.arch != "gpt2":
            raise ValueError("fused decode supports the gpt2 recipe only")
        if self.fused and (B > 64 or not lm_head):
            raise ValueError("fused decode needs batch <= 64 and lm_head")
        if self.fused and self.hd != 64:
            raise ValueError("fused decode supports head_dim 64 only")
        if self.fused and self.kv_pool is not None:
            raise ValueError("fused + paged not supported together yet")
        self._scale = 1.0 / float(np.sqrt(float(self.hd)))  # attention
        self.stream = self._C.hip.stream_create()
        self._graph = 0
        self._steps = 0
        # verify_chunk: buffers and captured graph per chunk size K
        self._chunk_bufs_by_k: Dict[int, Dict] = {}
        self._chunk_graphs: Dict[int, int] = {}
        # sample_tokens: per-slot parameters on the device, made on first use
        self._temps_dev = self._seeds_dev = None
        self._topk_dev = self._topp_dev = None

    # ------------------------------------------------------------ plumbing
    def _enqueue_fused(self):
        """Fused decode step: per layer [qkv(ADD_LN/EMBED_LN prologue +
        KV-scatter epilogue), attention, proj, ff1(ADD_LN + GeLU), ff2]
        + fused lm head — ~5 kernels/layer instead of 8."""
        C, s = self._C, self.stream
        B, Hd = self.batch, self.hidden
        ops = C.ops
        scale = 1.0 / float(np.sqrt(float(self.hd)))
        h_cur, h_nxt = self.h, self.h2
        for li, lay in enumerate(self.layers):
            if li == 0:  # embed + ln1 + qkv + kv scatter, persists h
                ops.decode_gemm_fused(
                    3, 2, x=0, r=0, h_out=h_cur.data_ptr(),
                    gamma=lay["ln1_g"].data_ptr(),
                    beta=lay["ln1_b"].data_ptr(),
                    B=lay["qkv_w"].data_ptr(), bias=lay["qkv_b"].data_ptr(),
                    C=self.qkv.data_ptr(), ids=self.ids.data_ptr(),
                    tok=self.tok.data_ptr(), posemb=self.posemb.data_ptr(),
                    pos=self.pos.data_ptr(),
                    kcache=lay["kcache"].data_ptr(),
                    vcache=lay["vcache"].data_ptr(), M=B, N=3 * Hd, K=Hd,
                    heads=self.heads, smax=self.smax, stream=s, sync=False)
            else:  # h_nxt = h_cur + ff2_out; qkv = ln1(h_nxt) @ W (+kv)
                ops.decode_gemm_fused(
                    2, 2, x=self.x2.data_ptr(), r=h_cur.data_ptr(),
                    h_out=h_nxt.data_ptr(), gamma=lay["ln1_g"].data_ptr(),
                    beta=lay["ln1_b"].data_ptr(),
                    B=lay["qkv_w"].data_ptr(), bias=lay["qkv_b"].data_ptr(),
                    C=self.qkv.data_ptr(), pos=self.pos.data_ptr(),
                    kcache=lay["kcache"].data_ptr(),
                    vcache=lay["vcache"].data_ptr(), M=B, N=3 * Hd, K=Hd,
                    heads=self.heads, smax=self.smax, stream=s, sync=False)
                h_cur, h_nxt = h_nxt, h_cur
            ops.decode_attention(self.qkv.data_ptr(),
                                 lay["kcache"].data_ptr(),
                                 lay["vcache"].data_ptr(),
                                 self.att.data_ptr(), self.pos.data_ptr(),
                                 B, self.heads, 1, self.smax, scale,
                                 stream=s, sync=False)
            ops.gemm_bt(0, self.att.data_ptr(), lay["proj_w"].data_ptr(),
                        self.x2.data_ptr(), bias=lay["proj_b"].data_ptr(),
                        M=B, N=Hd, K=Hd, epi=self._epi_bias, stream=s,
                        sync=False)
            # h_nxt = h_cur + proj_out; ff = gelu(ln2(h_nxt) @ W1)
            ops.decode_gemm_fused(
                2, 1, x=self.x2.data_ptr(), r=h_cur.data_ptr(),
                h_out=h_nxt.data_ptr(), gamma=lay["ln2_g"].data_ptr(),
                beta=lay["ln2_b"].data_ptr(), B=lay["ff1_w"].data_ptr(),
                bias=lay["ff1_b"].data_ptr(), C=self.ff.data_ptr(),
                pos=self.pos.data_ptr(), M=B, N=self.inter, K=Hd, stream=s,
                sync=False)
            h_cur, h_nxt = h_nxt, h_cur
            ops.gemm_bt(0, self.ff.data_ptr(), lay["ff2_w"].data_ptr(),
                        self.x2.data_ptr(), bias=lay["ff2_b"].data_ptr(),
                        M=B, N=Hd, K=self.inter, epi=self._epi_bias,
                        stream=s, sync=False)
        # head stays UNFUSED: at N=vocab the fused kernel's per-block LN
        # stats replicate across ~786 blocks (measured 102.6 vs 14.5 us,
        # tools/dbg_fused_perf) — add_layernorm + plain gemm_bt win there
        ops.add_layernorm(0, self.x2.data_ptr(), h_cur.data_ptr(),
                          self.lnf_g.data_ptr(), self.lnf_b.data_ptr(),
                          self.out.data_ptr(), M=B, N=Hd, stream=s,
                          sync=False)
        ops.gemm_bt(0, self.out.data_ptr(), self.tok.data_ptr(),
                    self.logits.data_ptr(), M=B, N=self.vocab, K=Hd,
                    epi=self._epi_none, stream=s, sync=False)
        ops.argmax_rows(self.logits.data_ptr(), self.gids.data_ptr(),
                        B, self.vocab, stream=s, sync=False)
        # no cross-step residual state: layer 0's EMBED prologue
        # regenerates the stream each step (h/h2 are just scratch)
        ops.advance_pos(self.pos.data_ptr(), B, self.smax, stream=s,
                        sync=False)

    def _kv(self, li: int, lay: Dict, qkv_ptr: int, rows: int,
            att_ptr: int = 0) -> None:
        """Per-layer KV append of `rows` rows per slot (1 = step, K =
        verify chunk) at pos[b] + row, then attention into att_ptr —
        dense caches or the paged pool. att_ptr = 0 is the prefill range
        writer: base position 0 (null pos), append only."""
        ops, s = self._C.ops, self.stream
        if self.kv_pool is not None:
            pool = self.kv_pool
            kc, vc = pool.kpools[li].data_ptr(), pool.vpools[li].data_ptr()
            table, mp = pool.table.data_ptr(), pool.max_pages
            sc = (pool.kscales[li], pool.vscales[li]) \
                if self._kv_format else None
        else:
            kc, vc = lay["kcache"].data_ptr(), lay["vcache"].data_ptr()
            table, mp = 0, 0
            sc = (lay["kscale"], lay["vscale"]) if self._kv_format else None
        # element format: fp16 (no scales) or mxfp8 codes + block scales
        fmt = dict(kscale=sc[0].data_ptr(), vscale=sc[1].data_ptr(),
                   kv_format=self._kv_format) if sc else {}
        ops.kv_append(qkv_ptr, kc, vc, self.batch, self.heads, rows,
                      self.smax, pos=self.pos.data_ptr() if att_ptr else 0,
                      table=table, max_pages=mp, stream=s, sync=False,
                      D=self.hd, kv_heads=self._nkv, **fmt)
        if att_ptr:
            ops.decode_attention(qkv_ptr, kc, vc, att_ptr,
                                 self.pos.data_ptr(), self.batch,
                                 self.heads, rows, self.smax, self._scale,
                                 table=table, max_pages=mp, stream=s,
                                 sync=False, D=self.hd, kv_heads=self._nkv,
                                 **fmt)

    @property
    def kv_cache_bytes(self) -> int:
        """Bytes of K/V storage behind this session: the dense caches
        (2 * layers * batch * kv_heads * smax rows) or the whole paged
        pool (2 * layers * num_pages * 64 * kv_heads rows), at
        kv_row_bytes(head_dim, kv_dtype) per row."""
        if self.kv_pool is not None:
            rows = self.kv_pool.num_pages * 64 * self.kv_heads
        else:
            rows = self.batch * self.kv_heads * self.smax
        return 2 * self.n_layers * rows * kv_row_bytes(self.hd,
                                                       self.kv_dtype)

    def _forward(self, b: Dict, kind: str, rows: int) -> None:
        """Record one transformer forward over batch*rows rows on the
        session stream (no syncs — capturable).

        b: the buffer roles `h` (residual stream, holds the embeddings on
        entry), `x`, `qkv`, `att`, `x2`, `ff`, `ff2` (LLaMA only) and
        `out`, where the final norm lands. `att` may alias `x`: `x` is
        dead once the qkv GEMM has read it.
        kind / rows per slot:
          "step"    1   at the device position pos[b]
          "chunk"   K   at pos[b] + row (chunk-strided RoPE)
          "prefill" Pp  at position row (null pos): KV append only, then
                        full-sequence causal attention
        The step is kernel-COUNT bound (~4.6 us graph-replay floor per
        kernel regardless of size - profiles/dec_kernel_stats), so every
        residual add is fused into the following norm (sum_out updates
        the residual stream in the same kernel)."""
        ops, s = self._C.ops, self.stream
        M, Hd, inter = self.batch * rows, self.hidden, self.inter
        llama = self.arch == "llama"
        prefill = kind == "prefill"
        h, x, qkv, att, x2, ff, out = (
            b[k].data_ptr() for k in ("h", "x", "qkv", "att", "x2", "ff",
                                      "out"))

        def gemm(a, w, c, N, K, bias=None, epi=self._epi_none):
            ops.gemm_bt(0, a, w.data_ptr(), c,
                        bias=bias.data_ptr() if bias is not None else 0,
                        M=M, N=N, K=K, epi=epi, stream=s, sync=False)

        def norm(src, g, beta, dst, res=0):
            """dst = norm(src); with res: res += src first, same kernel."""
            if llama and res:
                ops.add_rmsnorm(0, src, res, g.data_ptr(), dst, sum_out=res,
                                M=M, N=Hd, eps=self.rms_eps, stream=s,
                                sync=False)
            elif llama:
                ops.rmsnorm(0, src, g.data_ptr(), dst, M, Hd,
                            eps=self.rms_eps, stream=s, sync=False)
            elif res:
                ops.add_layernorm(0, src, res, g.data_ptr(),
                                  beta.data_ptr(), dst, sum_out=res, M=M,
                                  N=Hd, stream=s, sync=False)
            else:
                ops.layernorm(0, src, g.data_ptr(), beta.data_ptr(), dst, M,
                              Hd, stream=s, sync=False)

        def norm1(lay):
            return ((lay["rms1_g"], None) if llama
                    else (lay["ln1_g"], lay["ln1_b"]))

        norm(h, *norm1(self.layers[0]), x)
        for li, lay in enumerate(self.layers):
            if llama:
                gemm(x, lay["qkv_w"], qkv, self.qkv_w, Hd)
                # rotates at pos[b] (+ row in a chunk); prefill: at
                # row % rows (exact for rows < P; the padded tail is
                # causal-masked / overwritten before it is read)
                ops.rope(0, qkv, pos=0 if prefill else self.pos.data_ptr(),
                         M=M, S=rows if prefill else self.smax,
                         H=self.heads, D=self.hd, theta=self.theta,
                         stream=s, sync=False,
                         chunk=rows if kind == "chunk" else 0,
                         kv_heads=self._nkv)
            else:
                gemm(x, lay["qkv_w"], qkv, self.qkv_w, Hd, lay["qkv_b"],
                     self._epi_bias)
            if prefill:
                self._kv(li, lay, qkv, rows)
                ops.attention(0, qkv, att, self.batch, rows, self.heads,
                              self.hd, self._scale, stream=s, sync=False,
                              causal=1, kv_heads=self._nkv)
            else:
                self._kv(li, lay, qkv, rows, att)
            # h += proj; x = norm2(h); x2 = mlp(x)
            if llama:
                gemm(att, lay["proj_w"], x2, Hd, Hd)
                norm(x2, lay["rms2_g"], None, x, res=h)
                gemm(x, lay["gate_w"], ff, inter, Hd)
                gemm(x, lay["up_w"], b["ff2"].data_ptr(), inter, Hd)
                ops.silu_mul(0, ff, b["ff2"].data_ptr(), ff, M * inter,
                             stream=s, sync=False)
                gemm(ff, lay["down_w"], x2, Hd, inter)
            else:
                gemm(att, lay["proj_w"], x2, Hd, Hd, lay["proj_b"],
                     self._epi_bias)
                norm(x2, lay["ln2_g"], lay["ln2_b"], x, res=h)
                gemm(x, lay["ff1_w"], ff, inter, Hd, lay["ff1_b"],
                     self._epi_gelu)
                gemm(ff, lay["ff2_w"], x2, Hd, inter, lay["ff2_b"],
                     self._epi_bias)
            # h += mlp; x = the next layer's norm1(h), or out = final norm
            if li + 1 < self.n_layers:
                norm(x2, *norm1(self.layers[li + 1]), x, res=h)
            else:
                norm(x2, self.lnf_g, self.lnf_b, out, res=h)

    def _embed(self, ids, h, rows: int) -> None:
        """h = tok[ids] + posemb[pos[b] + row] for `rows` rows per slot."""
        self._C.ops.decode_embed(ids.data_ptr(), self.tok.data_ptr(),
                                 self.posemb.data_ptr(), h.data_ptr(),
                                 self.pos.data_ptr(), self.batch, rows,
                                 self.smax, self.hidden, stream=self.stream,
                                 sync=False)

    def _head(self, x, logits, gids, M: int) -> None:
        """Weight-tied lm head over M rows, then the greedy argmax ids."""
        ops, s = self._C.ops, self.stream
        ops.gemm_bt(0, x.data_ptr(), self.tok.data_ptr(), logits.data_ptr(),
                    M=M, N=self.vocab, K=self.hidden, epi=self._epi_none,
                    stream=s, sync=False)
        ops.argmax_rows(logits.data_ptr(), gids.data_ptr(), M, self.vocab,
                        stream=s, sync=False)

    def _enqueue(self):
        """Record one decode step's kernels on self.stream (pos-relative:
        embed / rope / kv_append / decode_attention all read the device
        counter, which the last kernel advances)."""
        if self.fused:
            self._enqueue_fused()
            return
        self._embed(self.ids, self.h, 1)
        self._forward(dict(h=self.h, x=self.x, qkv=self.qkv, att=self.att,
                           x2=self.x2, ff=self.ff, ff2=self.ff2,
                           out=self.out), "step", 1)
        if self.logits is not None:
            self._head(self.out, self.logits, self.gids, self.batch)
        self._C.ops.advance_pos(self.pos.data_ptr(), self.batch, self.smax,
                                stream=self.stream, sync=False)

    def prefill(self, prompt: np.ndarray) -> np.ndarray:
        """Fill the KV caches from a whole prompt [B, P] in ONE pass through
        the full-sequence kernels (causal online-softmax attention), then
        continue with step() from position P — prefill runs at the
        parallel-forward rate (~2M tok/s) instead of one replay per token.
        P is padded to the next multiple of 128 internally; the causal mask
        keeps positions < P exact and the padded cache slots are
        overwritten before they are ever attended. Returns the final
        hidden state at position P-1 per sequence. Must be called before
        the first step()."""
        import torch

        if self._steps != 0 or self._graph:
            raise RuntimeError("prefill must run before the first step()")
        prompt = np.ascontiguousarray(prompt, np.int32)
        B, P = prompt.shape
        assert B == self.batch and 0 < P < self.smax
        Pp = (P + 127) // 128 * 128
        if Pp > self.posemb.shape[0]:
            raise RuntimeError(
                f"prefill: padded prompt ({Pp}) exceeds the position table "
                f"({int(self.posemb.shape[0])}) — shorten the prompt or "
                "build the model with a longer seq")
        ids = np.zeros((B, Pp), np.int32)
        ids[:, :P] = prompt
        if self.kv_pool is not None:
            # map pages covering the PADDED prompt (the tail rows are
            # written by the range kv_append and overwritten by later
            # decode steps before they are ever attended)
            for b in range(B):
                for li in range((Pp - 1) // 64 + 1):
                    self.kv_pool.ensure(b, li)
        M = B * Pp
        Hd = self.hidden
        ops, s = self._C.ops, self.stream

        def act(width):
            return torch.empty(M, width, dtype=torch.half, device="cuda")

        dids = torch.from_numpy(ids.reshape(-1)).cuda()
        # three M x Hd buffers: attention writes into x, which is dead
        # once the qkv GEMM has read it
        h, x, x2 = act(Hd), act(Hd), act(Hd)
        bufs = dict(h=h, x=x, att=x, x2=x2, out=x, qkv=act(self.qkv_w),
                    ff=act(self.inter),
                    ff2=act(self.inter) if self.arch == "llama" else None)
        torch.cuda.synchronize()

        ops.embedding(0, dids.data_ptr(), self.tok.data_ptr(),
                      self.posemb.data_ptr(), out=h.data_ptr(), M=M, S=Pp,
                      H=Hd, stream=s, sync=False)
        self._forward(bufs, "prefill", Pp)
        self._C.hip.stream_synchronize(s)
        # x holds ln_f(h) for every position; hand back the last real one
        last = x.reshape(B, Pp, Hd)[:, P - 1].contiguous()
        torch.cuda.synchronize()
        self.pos.fill_(P)
        self._active[:] = True
        self._steps = P
        self._slot_steps[:] = P
        torch.cuda.synchronize()
        if self.logits is not None:
            ops.gemm_bt(0, last.data_ptr(), self.tok.data_ptr(),
                        self.logits.data_ptr(), M=B, N=self.vocab, K=Hd,
                        epi=self._epi_none, stream=s, sync=True)
            return self.logits.float().cpu().numpy()
        return last.float().cpu().numpy()

    def step(self, ids: np.ndarray,
             return_ids: bool = False) -> np.ndarray:
        """Feed one token per sequence; returns the final hidden state
        [B, hidden] fp32 (or logits [B, vocab] with lm_head=True). The
        device-side position counter starts at 0 and the captured graph
        advances it, so replays need no host-side position plumbing.

        return_ids=True (lm_head only): return the greedy argmax token
        per slot [B] int32 instead of logits — the argmax runs inside
        the captured graph, so only B ints cross PCIe per step."""
        if return_ids and self.logits is None:
            raise RuntimeError("return_ids requires lm_head=True")
        if self.kv_pool is not None:
            # map the page each active slot's next write lands in
            for b in range(self.batch):
                if self._active[b]:
                    self.kv_pool.ensure(b, int(self._slot_steps[b]) >> 6)
        if (self._slot_steps[self._active] >= self.smax).any():
            raise RuntimeError(
                "DecodeSession: a slot hit the sequence limit "
                "(reset_slot() it or end the session)")
        arr = np.ascontiguousarray(ids, np.int32)
        # synchronous H2D keeps the token copy ordered before the replay
        self._C.memory.memcpy_h2d(self.ids.data_ptr(), arr, arr.nbytes)
        if self._graph:
            self._C.hip.graph_launch(self._graph, self.stream)
        else:
            self._enqueue()
        self._C.hip.stream_synchronize(self.stream)
        if self.capture and not self._graph:
            # step 0 ran eagerly as the warm-up; now a fresh step is
            # RECORDED (capture does not execute) for replay from step 1
            self._C.hip.stream_begin_capture(self.stream)
            self._enqueue()
            self._graph = self._C.hip.stream_end_capture(self.stream)
        self._steps += 1
        self._slot_steps += 1
        if return_ids:
            return self.gids.cpu().numpy()
        if self.logits is not None:
            return self.logits.float().cpu().numpy()
        return self.out.float().cpu().numpy()

    # ------------------------------------------- speculative verification
    def _enqueue_chunk(self, cb: Dict, B: int, K: int) -> None:
        """Record one chunked-verification pass's kernels on the session
        stream (no syncs — capturable). All position dependence reads the
        device counter, so a captured chunk graph replays at any pos."""
        self._embed(cb["ids"], cb["h"], K)
        self._forward(dict(cb, out=cb["x"]), "chunk", K)
        self._head(cb["x"], cb["logits"], cb["gids"], B * K)

    def verify_chunk(self, tokens: np.ndarray,
                     greedy: bool = False) -> np.ndarray:
        """Score K proposed tokens per slot in ONE chunked forward
        (speculative decoding's verification step): tokens [B, K] are
        consumed at positions pos[b]..pos[b]+K-1 (their K/V overwrite any
        stale entries), and the TARGET logits for each position come back
        as [B, K, vocab] fp32. pos is NOT advanced — call add_pos() with
        the per-slot accepted counts. Requires lm_head=True.

        With capture=True the pass is hipGraph-captured PER CHUNK SIZE on
        first use and replayed afterwards (the measured spec-decode cost
        was eager per-kernel launch overhead; all position dependence is
        device-side, so one graph serves every position)."""
        import torch

        if self.logits is None:
            raise RuntimeError("verify_chunk requires lm_head=True")
        tokens = np.ascontiguousarray(tokens, np.int32)
        B, K = tokens.shape
        if self.kv_pool is not None:
            # map every page the chunk's writes land in (pos..pos+K-1)
            for b in range(self.batch):
                if self._active[b]:
                    p0 = int(self._slot_steps[b])
                    for li in range(p0 >> 6, ((p0 + K - 1) >> 6) + 1):
                        self.kv_pool.ensure(b, li)
        assert B == self.batch and K >= 1
        M = B * K
        Hd, inter = self.hidden, self.inter
        s = self.stream

        cb = self._chunk_bufs_by_k.get(K)
        if cb is None:
            cb = self._chunk_bufs_by_k[K] = dict(
                K=K,
                ids=torch.zeros(M, dtype=torch.int32, device="cuda"),
                h=torch.zeros(M, Hd, dtype=torch.half, device="cuda"),
                x=torch.zeros(M, Hd, dtype=torch.half, device="cuda"),
                x2=torch.zeros(M, Hd, dtype=torch.half, device="cuda"),
                qkv=torch.zeros(M, self.qkv_w, dtype=torch.half,
                                device="cuda"),
                att=torch.zeros(M, Hd, dtype=torch.half, device="cuda"),
                ff=torch.zeros(M, inter, dtype=torch.half, device="cuda"),
                ff2=(torch.zeros(M, inter, dtype=torch.half, device="cuda")
                     if self.arch == "llama" else None),
                logits=torch.zeros(M, self.vocab, dtype=torch.half,
                                   device="cuda"),
                gids=torch.zeros(M, dtype=torch.int32, device="cuda"),
            )
        self._C.memory.memcpy_h2d(cb["ids"].data_ptr(), tokens.reshape(-1),
                                  tokens.nbytes)
        if self.capture:
            gph = self._chunk_graphs.get(K)
            if gph is None:
                # first call: eager warm-up does the real work, then a
                # fresh pass is RECORDED (capture does not execute)
                self._enqueue_chunk(cb, B, K)
                self._C.hip.stream_synchronize(s)
                self._C.hip.stream_begin_capture(s)
                self._enqueue_chunk(cb, B, K)
                self._chunk_graphs[K] = self._C.hip.stream_end_capture(s)
            else:
                self._C.hip.graph_launch(gph, s)
                self._C.hip.stream_synchronize(s)
        else:
            self._enqueue_chunk(cb, B, K)
            self._C.hip.stream_synchronize(s)
        if greedy:
            return cb["gids"].cpu().numpy().reshape(B, K)
        return cb["logits"].float().cpu().numpy().reshape(B, K, self.vocab)

    def sample_tokens(self, temps: np.ndarray, seeds: np.ndarray,
                      top_k: Optional[np.ndarray] = None,
                      top_p: Optional[np.ndarray] = None) -> np.ndarray:
        """Device-side temperature sampling of the LAST step's logits
        (Gumbel-max: an exact softmax(logits/T) categorical draw per
        slot; temps[b] <= 0 degrades to greedy argmax). Noise is keyed
        (seeds[b], device pos[b], index), so consecutive steps draw
        fresh noise and a (seed, position) pair replays identically.
        Only B ints cross PCIe.

        top_k / top_p (per-slot int32 / float32 arrays, either may be
        None = off for every slot) restrict each slot's draw to its
        top-k / nucleus candidate set on the device
        (ops.topk_topp_sample_rows; the rule is engine/sampling.py's
        truncation_reference). A slot with top_k[b] <= 0 and top_p[b]
        outside (0, 1) draws exactly what it draws with both None."""
        if self.logits is None:
            raise RuntimeError("sample_tokens requires lm_head=True")
        torch = self._torch
        if self._temps_dev is None:
            self._temps_dev = torch.zeros(self.batch, dtype=torch.float32,
                                          device="cuda")
            self._seeds_dev = torch.zeros(self.batch, dtype=torch.int32,
                                          device="cuda")
        self._C.memory.memcpy_h2d(self._temps_dev.data_ptr(),
                                  np.ascontiguousarray(temps, np.float32),
                                  self.batch * 4)
        self._C.memory.memcpy_h2d(self._seeds_dev.data_ptr(),
                                  np.ascontiguousarray(seeds, np.int32),
                                  self.batch * 4)
        if top_k is None and top_p is None:
            self._C.ops.gumbel_argmax_rows(
                self.logits.data_ptr(), self.gids.data_ptr(),
                temps=self._temps_dev.data_ptr(),
                seeds=self._seeds_dev.data_ptr(), pos=self.pos.data_ptr(),
                M=self.batch, V=self.vocab, stream=self.stream, sync=True)
            return self.gids.cpu().numpy()
        if self._topk_dev is None:
            self._topk_dev = torch.zeros(self.batch, dtype=torch.int32,
                                         device="cuda")
            self._topp_dev = torch.zeros(self.batch, dtype=torch.float32,
                                         device="cuda")
        top_k = np.ascontiguousarray(
            np.zeros(self.batch) if top_k is None else top_k, np.int32)
        top_p = np.ascontiguousarray(
            np.zeros(self.batch) if top_p is None else top_p, np.float32)
        if top_k.size != self.batch or top_p.size != self.batch:
            raise ValueError("top_k / top_p need one entry per slot")
        self._C.memory.memcpy_h2d(self._topk_dev.data_ptr(), top_k,
                                  self.batch * 4)
        self._C.memory.memcpy_h2d(self._topp_dev.data_ptr(), top_p,
                                  self.batch * 4)
        self._C.ops.topk_topp_sample_rows(
            self.logits.data_ptr(), self.gids.data_ptr(),
            temps=self._temps_dev.data_ptr(),
            top_k=self._topk_dev.data_ptr(),
            top_p=self._topp_dev.data_ptr(),
            seeds=self._seeds_dev.data_ptr(), pos=self.pos.data_ptr(),
            M=self.batch, V=self.vocab, stream=self.stream, sync=True)
        return self.gids.cpu().numpy()

    def get_pos(self) -> np.ndarray:
        """Per-slot positions from the HOST mirror (no D2H round-trip:
        device pos only changes via step()'s advance kernel — mirrored
        by _slot_steps — or via these host-side setters)."""
        return np.where(self._active, self._slot_steps, -1).astype(np.int32)

    def add_pos(self, counts: np.ndarray) -> None:
        """Advance each slot's position by counts[b] (speculative
        acceptance: the chunk's first counts[b] tokens are now consumed)."""
        counts = np.asarray(counts, np.int64)
        cur = self.get_pos().astype(np.int64)
        new = np.where(cur >= 0, np.minimum(cur + counts, self.smax - 1),
                       cur)
        self.pos.copy_(self._torch.from_numpy(new.astype(np.int32)).cuda())
        self._slot_steps = np.where(cur >= 0,
                                    self._slot_steps + counts,
                                    self._slot_steps)
        self._torch.cuda.synchronize()

    def set_pos(self, positions: np.ndarray) -> None:
        """Set per-slot absolute positions (speculative rollback of a
        draft session to the target's accepted frontier)."""
        arr = np.ascontiguousarray(positions, np.int32)
        self.pos.copy_(self._torch.from_numpy(arr).cuda())
        self._slot_steps = arr.astype(np.int64).clip(min=0)
        self._active = arr >= 0
        self._torch.cuda.synchronize()

    def reset_slot(self, b: int) -> None:
        """Restart slot b at position 0 (continuous batching in lockstep:
        the next step() token for this slot begins a fresh sequence while
        the other slots keep decoding against their caches)."""
        self.pos[b] = 0
        self._slot_steps[b] = 0
        self._active[b] = True
        if self.kv_pool is not None:
            self.kv_pool.free_slot(b)  # fresh sequence: recycle its pages
        self._torch.cuda.synchronize()

    def idle_slot(self, b: int) -> None:
        """Park slot b (no active request): pos[b] = -1 makes every
        per-slot decode kernel early-exit for it, so an empty slot in the
        continuous batch costs ~nothing per replayed step. reset_slot(b)
        re-activates it for a fresh sequence."""
        self.pos[b] = -1
        self._slot_steps[b] = 0
        self._active[b] = False
        if self.kv_pool is not None:
            self.kv_pool.free_slot(b)  # parked slots hold ZERO cache pages
        self._torch.cuda.synchronize()

    def close(self):
        if self._graph:
            self._C.hip.graph_destroy(self._graph)
            self._graph = 0
        for g in self._chunk_graphs.values():
            self._C.hip.graph_destroy(g)
        self._chunk_graphs = {}

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class SpeculativeDecoder:
    """Greedy speculative decoding over two DecodeSessions (beyond-
    reference serving capability): a cheap DRAFT model proposes k tokens
    per round, the TARGET verifies all k in ONE chunked forward
    (verify_chunk), and the longest matching prefix is accepted plus the
    target's own correction token. The emitted stream is IDENTICAL to
    greedy decoding with the target alone — the draft only changes speed,
    never output (the invariant the GPU test checks with a mismatched
    draft). Per-slot positions let different slots accept different
    lengths each round.

    Both sessions need lm_head=True and the same vocab; prime both on the
    same context before generate().
    """

    def __init__(self, target: "DecodeSession", draft: "DecodeSession",
                 k: int = 4):
        if target.logits is None or draft.logits is None:
            raise ValueError("both sessions need lm_head=True")
        if target.vocab != draft.vocab or target.batch != draft.batch:
            raise ValueError("vocab/batch mismatch between target and draft")
        self.target = target
        self.draft = draft
        self.k = k
        self.proposed = 0
        self.accepted = 0

    def generate(self, seed: np.ndarray, steps: int):
        """Greedy-generate `steps` tokens per slot after consuming `seed`
        [B]. Returns (tokens [B, steps] int32, acceptance_rate)."""
        B, k = self.target.batch, self.k
        seed = np.ascontiguousarray(seed, np.int32)
        # ids-only verification (greedy=True): argmax happens on-device,
        # so only token ids ever cross PCIe (B*k ints vs B*k*vocab floats)
        gt = self.target.verify_chunk(seed[:, None], greedy=True)[:, 0]
        self.target.add_pos(np.ones(B, np.int64))
        gd = self.draft.verify_chunk(seed[:, None], greedy=True)[:, 0]
        self.draft.add_pos(np.ones(B, np.int64))

        out = [[] for _ in range(B)]
        while min(len(o) for o in out) < steps:
            # ---- draft chain: k greedy proposals ----
            props = np.zeros((B, k), np.int32)
            cur = gd.astype(np.int32)
            for i in range(k):
                props[:, i] = cur
                gd = self.draft.verify_chunk(cur[:, None],
                                             greedy=True)[:, 0]
                self.draft.add_pos(np.ones(B, np.int64))
                cur = gd.astype(np.int32)
            # ---- target verifies the whole chunk at once ----
            tg = self.target.verify_chunk(props, greedy=True)  # [B, k]
            accept = np.zeros(B, np.int64)
            corr = np.zeros(B, np.int32)
            for b in range(B):
                g = int(gt[b])
                a = 0
                while a < k and props[b, a] == g:
                    out[b].append(g)
                    g = int(tg[b, a])
                    a += 1
                accept[b] = a
                corr[b] = g          # target's own next token
                out[b].append(g)
            self.proposed += B * k
            self.accepted += int(accept.sum())
            # ---- advance target past the accepted prefix, consume the
            # correction token (its K/V overwrites the rejected slot) ----
            self.target.add_pos(accept)
            gt = self.target.verify_chunk(corr[:, None], greedy=True)[:, 0]
            self.target.add_pos(np.ones(B, np.int64))
            # ---- roll the draft back to the target's frontier ----
            self.draft.set_pos(self.target.get_pos() - 1)
            gd = self.draft.verify_chunk(corr[:, None], greedy=True)[:, 0]
            self.draft.add_pos(np.ones(B, np.int64))
        rate = self.accepted / max(self.proposed, 1)
        return (np.array([o[:steps] for o in out], np.int32), rate)
