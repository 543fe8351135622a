"""Top-k / nucleus truncation: the rule, as a pure-numpy reference.

This module is the definition that `ops.topk_topp_sample_rows` (the
device kernel, csrc/kernels/sampling.hip) and its tests are held to.

For T > 0 let p = softmax(x / T) over the row, x being the fp16 logits
read as real numbers with -0.0 treated as +0.0. Tokens are grouped into
VALUE CLASSES v_1 > v_2 > ... (equal logits form one class) and classes
are walked from the top:

* top_k keeps classes up to the first one at which the cumulative token
  count reaches top_k (top_k <= 0 or top_k >= V: off);
* top_p keeps classes up to the first one at which the cumulative
  probability reaches top_p (active only for 0 < top_p < 1);
* with both, the stricter (higher) threshold wins;
* the top class is always kept, and a class is never split.

So the kept set is `x >= thr` for one threshold value: a function of the
values alone, with no index tie rule, invariant under permutation. Without
ties at the cut it is the candidate set of GenerationEngine._sample. The
draw is categorical over the kept set with renormalised p.

-inf logits (masked tokens) weigh 0. While a filter is active they form no
class, so they are never kept (a row of nothing but -inf is out of scope).
With no filter active nothing is cut: thr = -inf and kept = V.

temperature <= 0 is greedy: the lowest-index argmax alone, whatever
top_k / top_p say (kept = 1, thr = the row maximum).
"""
from __future__ import annotations

import numpy as np


def truncation_reference(logits_fp16_row, temperature: float, top_k: int,
                         top_p: float):
    """-> (thr: float, kept: int, mask: bool[V]) for one row of logits."""
    x = np.asarray(logits_fp16_row, np.float16).astype(np.float64).ravel()
    x = x + 0.0  # -0.0 -> +0.0
    V = x.shape[0]
    if temperature <= 0.0:
        mask = np.zeros(V, bool)
        mask[int(np.argmax(x))] = True
        return float(x.max()), 1, mask
    use_k = 0 < top_k < V
    use_p = 0.0 < top_p < 1.0
    if not (use_k or use_p):
        return float("-inf"), V, np.ones(V, bool)
    finite = x[x > -np.inf]
    vals, counts = np.unique(finite, return_counts=True)
    vals, counts = vals[::-1], counts[::-1]  # classes, highest first
    with np.errstate(invalid="ignore"):
        w = np.exp((vals - vals[0]) / temperature) * counts
    cut = len(vals) - 1
    if use_k:
        cut = min(cut, int(np.searchsorted(np.cumsum(counts), top_k)))
    if use_p:
        cum = np.cumsum(w) / w.sum()
        cut = min(cut, int(np.searchsorted(cum, top_p)))
    thr = float(vals[cut])
    mask = x >= thr
    return thr, int(mask.sum()), mask
