"""Serving-side generation for the Mixtral (MoE) family.

The passes of ``models/generate.py`` serve Mixtral as they serve Llama:
the attention half of a Mixtral block is identical, so it runs the same
kernels (in decode: skinny-M GEMV, decode_rope_cache, split-K
flash-decode attention, rmsnorm_res), and the passes pick the MLP half
by the block. The ``*_moe`` names here are aliases of those passes, kept
for callers that import them; batchers need no function arguments for a
Mixtral model. What is Mixtral's own is the decode MLP half below: top-k
expert routing where, at decode batch B, every (token, expert) group
runs the fused GEMV+SwiGLU expert FFN on its tokens only, so each step
streams just the ACTIVE experts' weights (<= B*top_k of num_experts per
layer). In prefill the MLP half is the training ``MoELayer`` itself.

Single-rank serving only (``ep_size == 1`` — all experts local); the
expert-parallel all-to-all path in models/mixtral.py is a training
construct. Eager-only: MoE routing is data-dependent, so a hipGraph
capture would freeze one routing decision — the dense-model
``GraphedDecoder`` has no MoE counterpart by design.
"""

from __future__ import annotations

import torch

from torchx_amd import ops

from .generate import (
    KVCache, decode_step, generate, prefill, prefill_extend, prefill_ragged,
)
from .mixtral import MoELayer

__all__ = ["prefill_moe", "prefill_extend_moe", "prefill_ragged_moe",
           "decode_step_moe", "generate_moe", "KVCache"]


def _moe_mlp_decode(moe: MoELayer, x: torch.Tensor) -> torch.Tensor:
    """Top-k MoE for a decode micro-batch x [B, H] -> [B, H]; experts run
    the skinny-M GEMV + fused SwiGLU path on their assigned tokens."""
    assert moe.ep_size == 1, "serving path is single-rank (all experts local)"
    cfg = moe.cfg
    logits = (x @ moe.router.weight.t()).float()          # [B, E]
    w, idx = torch.topk(logits, cfg.top_k, dim=-1)
    w = torch.softmax(w, dim=-1).to(x.dtype)              # [B, k]
    idx_h = idx.cpu()  # ONE host sync per layer; partitioning is host-side
    out = torch.zeros_like(x)
    for e in range(cfg.num_experts):
        rows_h = (idx_h == e).any(-1).nonzero(as_tuple=True)[0]
        if rows_h.numel() == 0:
            continue
        rows = rows_h.to(x.device, non_blocking=True)
        exp = moe.local_experts[e]
        h = ops.decode_linear_swiglu(x[rows], exp.wgu.weight)
        ye = ops.decode_linear(h, exp.wdown.weight)
        coef = (w * (idx == e)).sum(-1)[rows]             # [n], on device
        out[rows] += ye * coef[:, None]
    return out


# the shared passes tell a MixtralBlock from a LlamaBlock themselves
prefill_moe = prefill
prefill_extend_moe = prefill_extend
prefill_ragged_moe = prefill_ragged
decode_step_moe = decode_step
generate_moe = generate
