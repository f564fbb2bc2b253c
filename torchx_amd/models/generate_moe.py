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
layer). Router, top-k and softmax run on the device and
``ops.moe_decode_mlp`` reads their result there: its two grouped expert
GEMV kernels (ops/csrc/moe_gemv.hip) are the whole MLP half, with no
host sync (``ops.set_moe_decode_impl("loop")`` brings back the
per-expert loop with its one sync per layer; same bits).
``ops.set_moe_router_impl("fused")`` moves router, top-k and softmax into
the kernel of the norm in front of them (``ops.rmsnorm_res_route``,
ops/csrc/moe_route.hip). In prefill the MLP half is the training
``MoELayer`` itself.

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
    KVCache, _decode_w, decode_step, generate, prefill, prefill_extend,
    prefill_ragged,
)
from .mixtral import MoELayer

__all__ = ["prefill_moe", "prefill_extend_moe", "prefill_ragged_moe",
           "decode_step_moe", "generate_moe", "KVCache"]


def _expert_weights(moe: MoELayer):
    """The experts' (wgu, wdown) weight lists, built once per layer. They
    hold the parameters themselves (no copy, no stacking), which ``.to()``
    and ``load_state_dict`` update in place — or the experts' fp8
    ``decode_weight`` where ``quantize_decode_weights`` made them; it drops
    the cached lists, and so does a change in whether the experts have
    one."""
    fp8 = hasattr(moe.local_experts[0].wgu, "decode_weight")
    cached = moe.__dict__.get("_decode_weights")
    if cached is None or cached[0] != fp8:
        cached = (fp8, [_decode_w(e.wgu) for e in moe.local_experts],
                  [_decode_w(e.wdown) for e in moe.local_experts])
        moe.__dict__["_decode_weights"] = cached
    return cached[1:]


def _moe_mlp_decode(moe: MoELayer, x: torch.Tensor) -> torch.Tensor:
    """Top-k MoE for a decode micro-batch x [B, H] -> [B, H]: the routing
    stays on the device and ``ops.moe_decode_mlp`` runs the chosen experts'
    FFNs on their tokens."""
    assert moe.ep_size == 1, "serving path is single-rank (all experts local)"
    cfg = moe.cfg
    logits = (x @ moe.router.weight.t()).float()          # [B, E]
    w, idx = torch.topk(logits, cfg.top_k, dim=-1)
    w = torch.softmax(w, dim=-1).to(x.dtype)              # [B, k]
    return ops.moe_decode_mlp(x, idx, w, *_expert_weights(moe))


def _moe_norm_mlp_decode(blk, x: torch.Tensor, a: torch.Tensor, eps: float):
    """``decode_step``'s residual add + MLP norm + MoE MLP of a Mixtral
    block under ``ops.set_moe_router_impl("fused")``: x, a [B, H] -> (the
    new residual stream, the MLP output). Three dispatches: the norm and
    the routing are one kernel (fp32 logits, ties to the lower expert),
    which ``ops.moe_decode_mlp`` reads on the device."""
    moe = blk.moe
    assert moe.ep_size == 1, "serving path is single-rank (all experts local)"
    x, xn, idx, cw = ops.rmsnorm_res_route(x, a, blk.mlp_norm, eps,
                                           moe.router.weight, moe.cfg.top_k)
    return x, ops.moe_decode_mlp(xn, idx, cw, *_expert_weights(moe))


# the shared passes tell a MixtralBlock from a LlamaBlock themselves
prefill_moe = prefill
prefill_extend_moe = prefill_extend
prefill_ragged_moe = prefill_ragged
decode_step_moe = decode_step
generate_moe = generate
