"""Serving-side generation for the Llama and Mixtral families: prefill +
KV-cache decode on the CDNA4 kernels. One body per kind of pass serves
both; ``_mlp_prefill`` / ``_mlp_decode`` hold what differs.

The training path never materializes K/V (the fused qkv attention keeps
them inside the kernel), so generation runs its own per-layer loop over
the SAME module weights: prefill uses the rope + flash-attention kernels
and captures the roped K/V into the cache; every decode step runs the
single-position ``ops.decode_attention`` kernel (flash-decode style)
against the cache. Inference only — ``torch.no_grad`` throughout.

No analog exists in the reference (a launcher); this is the
"deployment and serving" side of the bundled MI355X reference app.
288 GB HBM3E fits very large caches: a Llama-3-8B KV cache is
B * S * 8 heads * 128 * 2 (k+v) * 2 bytes = 8 KB per token-row
(~1 GB at B=4, S=32k).
"""

from __future__ import annotations

import itertools
from collections import ChainMap
from dataclasses import dataclass
from typing import Optional

import torch

from torchx_amd import ops

from .llama import LlamaConfig, LlamaModel


@dataclass
class KVCache:
    k: torch.Tensor  # [B, T, Hkv, 128] bf16
    v: torch.Tensor
    length: int = 0

    @staticmethod
    def empty(cfg: LlamaConfig, batch: int, max_len: int,
              device: torch.device) -> "KVCache":
        shape = (batch, max_len, cfg.num_kv_heads, cfg.head_dim)
        return KVCache(
            k=torch.zeros(shape, dtype=torch.bfloat16, device=device),
            v=torch.zeros(shape, dtype=torch.bfloat16, device=device),
        )


class OutOfPages(RuntimeError):
    """The page pool cannot supply the pages a request needs."""


class PageAllocator:
    """Host-side free list over the physical pages of a paged KV pool.
    Page 0 is reserved as the dump page (inactive batch rows read and
    write only its slot 0) and is never handed out. The free list is
    LIFO, so a run is deterministic and a freed page goes straight to the
    next request.

    Pages are reference counted for prefix sharing: ``alloc`` hands a page
    to its first holder, ``share`` adds a holder, ``free`` drops one, and
    the page returns to the free list when its last holder frees it.
    Without ``share`` calls every page has one holder and the behaviour is
    the plain free list's."""

    def __init__(self, num_pages: int):
        assert num_pages >= 2, "need the dump page plus one usable page"
        self.num_pages = num_pages
        # popped from the end: page 1 is handed out first
        self._free = list(range(num_pages - 1, 0, -1))
        self._is_free = [True] * num_pages
        self._is_free[0] = False
        self._refs = [0] * num_pages  # holders per page

    @property
    def num_free(self) -> int:
        return len(self._free)

    def alloc(self, n: int) -> list:
        """``n`` pages, all or nothing."""
        if n > len(self._free):
            raise OutOfPages(f"need {n} pages, {len(self._free)} free")
        pages = [self._free.pop() for _ in range(n)]
        for p in pages:
            self._is_free[p] = False
            self._refs[p] = 1
        return pages

    def share(self, pages) -> None:
        """Add one holder to each of ``pages`` (all must be held)."""
        for p in pages:
            assert 0 < p < self.num_pages, f"no such page {p}"
            assert not self._is_free[p], f"page {p} is not held"
        for p in pages:
            self._refs[p] += 1

    def refcount(self, p: int) -> int:
        """Number of holders of page ``p`` (0 for a free page)."""
        return self._refs[p]

    def free(self, pages) -> None:
        """Drop one holder of each page; the last one frees it."""
        for p in pages:
            assert p != 0, "page 0 is the dump page"
            assert 0 < p < self.num_pages, f"no such page {p}"
            assert not self._is_free[p], f"double free of page {p}"
            self._refs[p] -= 1
            if self._refs[p] == 0:
                self._is_free[p] = True
                self._free.append(p)


@dataclass
class PagedKVCache:
    """One layer's paged KV pool. ``block_table`` (int32 [B, M]) is shared
    by every layer: logical page j of sequence b lives in physical page
    ``block_table[b, j]`` of each layer's pool. ``row`` narrows the cache
    to one batch row for a [1, S] prefill (see ``for_row``)."""
    kpool: torch.Tensor  # [num_pages, P, Hkv, D] bf16
    vpool: torch.Tensor
    block_table: torch.Tensor
    row: Optional[int] = None

    @staticmethod
    def empty(cfg: LlamaConfig, num_pages: int, page_size: int,
              block_table: torch.Tensor,
              device: torch.device) -> "PagedKVCache":
        assert 16 <= page_size <= 256 and page_size & (page_size - 1) == 0
        shape = (num_pages, page_size, cfg.num_kv_heads, cfg.head_dim)
        return PagedKVCache(
            kpool=torch.zeros(shape, dtype=torch.bfloat16, device=device),
            vpool=torch.zeros(shape, dtype=torch.bfloat16, device=device),
            block_table=block_table,
        )

    @property
    def page_size(self) -> int:
        return self.kpool.shape[1]

    def for_row(self, row: int) -> "PagedKVCache":
        return PagedKVCache(self.kpool, self.vpool, self.block_table, row)

    def store_prefix(self, k: torch.Tensor, v: torch.Tensor) -> None:
        """Scatter a prefilled prefix into the pages of its row(s):
        k, v [1, S, Hkv, D] go to row ``self.row``; without a row,
        [B, S, Hkv, D] go to rows 0..B-1. Plain torch plumbing (one
        index_copy_ per pool), no host sync."""
        P = self.page_size
        B, S = k.shape[:2]
        r0 = 0 if self.row is None else self.row
        assert self.row is None or B == 1
        t = torch.arange(S, device=self.block_table.device)
        table = self.block_table[r0:r0 + B]
        slots = (table[:, t // P].long() * P + t % P).reshape(-1)
        kflat = self.kpool.view(-1, *self.kpool.shape[2:])
        vflat = self.vpool.view(-1, *self.vpool.shape[2:])
        kflat.index_copy_(0, slots, k.reshape(B * S, *k.shape[2:]))
        vflat.index_copy_(0, slots, v.reshape(B * S, *v.shape[2:]))

    def store_rows(self, k: torch.Tensor, v: torch.Tensor,
                   start: int) -> None:
        """``store_prefix`` at an offset: k, v [B, S, Hkv, D] become the
        logical rows ``start .. start+S-1`` of the same row(s)."""
        P = self.page_size
        B, S = k.shape[:2]
        t = torch.arange(start, start + S, device=self.block_table.device)
        table = self.table_rows(B)
        slots = (table[:, t // P].long() * P + t % P).reshape(-1)
        kflat = self.kpool.view(-1, *self.kpool.shape[2:])
        vflat = self.vpool.view(-1, *self.vpool.shape[2:])
        kflat.index_copy_(0, slots, k.reshape(B * S, *k.shape[2:]))
        vflat.index_copy_(0, slots, v.reshape(B * S, *v.shape[2:]))

    def table_rows(self, batch: int) -> torch.Tensor:
        """The block-table row(s) a [batch, S] prefill of this cache
        addresses, selected as ``store_prefix`` selects them."""
        r0 = 0 if self.row is None else self.row
        assert self.row is None or batch == 1
        return self.block_table[r0:r0 + batch]


def _split_qkv(qkv: torch.Tensor, cfg: LlamaConfig):
    B, S, _ = qkv.shape
    q, k, v = qkv.split([cfg.q_dim, cfg.kv_dim, cfg.kv_dim], dim=-1)
    return (q.reshape(B, S, cfg.num_heads, cfg.head_dim).contiguous(),
            k.reshape(B, S, cfg.num_kv_heads, cfg.head_dim).contiguous(),
            v.reshape(B, S, cfg.num_kv_heads, cfg.head_dim).contiguous())


def _mlp_prefill(blk, xn: torch.Tensor) -> torch.Tensor:
    """MLP half of a block in a prefill pass: normed activations in, the
    block's MLP output out. With ``_mlp_decode`` this is all the serving
    passes know about the model family: a MixtralBlock has ``moe``, a
    LlamaBlock has ``wgu`` / ``wdown``."""
    if "moe" in blk._modules:
        return blk.moe(xn)
    return blk.wdown(ops.swiglu_packed(blk.wgu(xn)))


def _mlp_decode(blk, xn: torch.Tensor) -> torch.Tensor:
    """``_mlp_prefill`` for a decode micro-batch xn [B, H] -> [B, H]. A
    Python branch taken while the step is recorded, so a hipGraph capture
    of the dense step holds only the two GEMVs."""
    if "moe" in blk._modules:
        # generate_moe imports this module
        from .generate_moe import _moe_mlp_decode
        return _moe_mlp_decode(blk.moe, xn)
    return ops.decode_linear(ops.decode_linear_swiglu(xn, blk.wgu.weight),
                             blk.wdown.weight)


def _prefill_pass(model, tokens: torch.Tensor, caches: list, start: int,
                  attend) -> torch.Tensor:
    """Body of the [B, S] prefill passes, tokens at positions
    ``start .. start+S-1``. The attention half of a block is norm, wqkv,
    both ropes, ``attend(cache, q, k, v)`` — which puts the roped K/V
    where the pass keeps them and runs its attention op — and wo +
    residual. Returns the last position's logits [B, vocab]."""
    cfg = model.cfg
    B, S = tokens.shape
    cos = model.rope_cos[start:start + S]
    sin = model.rope_sin[start:start + S]
    x = model.embed(tokens)
    for blk, cache in zip(model.blocks, caches):
        xn = ops.rmsnorm(x, blk.attn_norm, cfg.rms_eps)
        q, k, v = _split_qkv(blk.wqkv(xn), cfg)
        q = ops.rope(q, cos, sin)
        k = ops.rope(k, cos, sin)
        attn = attend(cache, q, k, v)
        x = x + blk.wo(attn.reshape(B, S, cfg.q_dim))
        xn = ops.rmsnorm(x, blk.mlp_norm, cfg.rms_eps)
        x = x + _mlp_prefill(blk, xn)
    x = ops.rmsnorm(x, model.final_norm, cfg.rms_eps)
    return model.lm_head(x[:, -1])


@torch.no_grad()
def prefill(model, tokens: torch.Tensor, caches: list) -> torch.Tensor:
    """Run the prompt through the model (Llama or Mixtral), filling
    per-layer KV caches of either kind; attention is the dense training
    kernel. Returns the last position's logits [B, vocab]."""
    S = tokens.shape[1]

    def attend(cache, q, k, v):
        if isinstance(cache, PagedKVCache):
            cache.store_prefix(k, v)
        else:
            cache.k[:, :S] = k
            cache.v[:, :S] = v
            cache.length = S
        return ops.flash_attention(q, k, v, causal=True)

    return _prefill_pass(model, tokens, caches, 0, attend)


@torch.no_grad()
def prefill_extend(model, tokens: torch.Tensor, caches: list,
                   ctx: int) -> torch.Tensor:
    """Prefill a piece of a prompt behind ``ctx`` rows the paged caches
    already hold: tokens [B, S] sit at positions ctx .. ctx+S-1. Their
    roped K/V go into the pages (``store_rows``) and attention runs over
    the block table (``ops.paged_prefill_attention``), so the cached rows
    are neither recomputed nor copied. Returns the last position's logits
    [B, vocab]. ``ctx = 0`` with the whole prompt is a paged ``prefill``."""
    B, S = tokens.shape
    assert ctx >= 0 and S >= 1
    assert ctx + S <= model.rope_cos.shape[0], "beyond the rope tables"
    ctx_dev = torch.full((B,), ctx, dtype=torch.int32, device=tokens.device)

    def attend(cache, q, k, v):
        assert isinstance(cache, PagedKVCache), "paged caches only"
        assert ctx + S <= cache.block_table.shape[1] * cache.page_size, \
            "beyond the block table"
        cache.store_rows(k, v, ctx)
        return ops.paged_prefill_attention(q, cache.kpool, cache.vpool,
                                           cache.table_rows(B), ctx_dev)

    return _prefill_pass(model, tokens, caches, ctx, attend)


@dataclass
class RaggedPass:
    """What one ragged prefill pass works out once and every layer reuses:
    per packed token its logical position and physical pool row, per
    sequence its cached length and block-table row, the attention launch
    plan, and the packed index of each sequence's last token."""
    q_lens: list
    pos: torch.Tensor    # int32 [T]
    slot: torch.Tensor   # int32 [T]
    ctx: torch.Tensor    # int32 [B]
    table: torch.Tensor  # int32 [B, M]
    plan: "ops.RaggedPlan"
    last: torch.Tensor   # int64 [B]

    @staticmethod
    def build(model, caches: list, rows, q_lens, ctx,
              device: torch.device) -> "RaggedPass":
        q_lens = [int(n) for n in q_lens]
        ctx = [int(c) for c in ctx]
        assert len(rows) == len(q_lens) == len(ctx) >= 1
        assert min(q_lens) >= 1 and min(ctx) >= 0
        cache = caches[0]
        assert isinstance(cache, PagedKVCache), "paged caches only"
        P = cache.page_size
        ends = [c + n for c, n in zip(ctx, q_lens)]
        assert max(ends) <= model.rope_cos.shape[0], "beyond the rope tables"
        assert max(ends) <= cache.block_table.shape[1] * P, \
            "beyond the block table"
        # host lists -> one small copy each, no device sync
        seq = [b for b, n in enumerate(q_lens) for _ in range(n)]
        pos = [c + i for c, n in zip(ctx, q_lens) for i in range(n)]
        plan = ops.RaggedPlan(q_lens, device, ctx=ctx)

        def dev(v, dtype):
            return torch.tensor(v, dtype=dtype, device=device)

        table = cache.block_table[dev(list(rows), torch.long)]
        pos_l = dev(pos, torch.long)
        slot = table[dev(seq, torch.long), pos_l // P].long() * P + pos_l % P
        return RaggedPass(q_lens, pos_l.int(), slot.int(),
                          dev(ctx, torch.int32), table.contiguous(), plan,
                          dev([e - 1 for e in plan.cu[1:]], torch.long))


def _ragged_attention(model, blk, cache: PagedKVCache, x: torch.Tensor,
                      rp: RaggedPass) -> torch.Tensor:
    """Attention half of a block over packed tokens x [1, T, H]: rope and
    page append in one dispatch, ragged attention over the block table."""
    cfg = model.cfg
    assert isinstance(cache, PagedKVCache), "paged caches only"
    T = x.shape[1]
    xn = ops.rmsnorm(x, blk.attn_norm, cfg.rms_eps)
    q = ops.paged_prefill_rope_cache(
        blk.wqkv(xn).reshape(T, -1), cache.kpool, cache.vpool,
        model.rope_cos, model.rope_sin, rp.pos, rp.slot, cfg.num_heads)
    attn = ops.paged_prefill_attention_ragged(
        q, cache.kpool, cache.vpool, rp.table, rp.q_lens, rp.ctx,
        plan=rp.plan)
    return x + blk.wo(attn.reshape(1, T, cfg.q_dim))


def _ragged_logits(model, x: torch.Tensor, rp: RaggedPass) -> torch.Tensor:
    x = ops.rmsnorm(x[:, rp.last], model.final_norm, model.cfg.rms_eps)
    return model.lm_head(x)[0]


@torch.no_grad()
def prefill_ragged(model, tokens: torch.Tensor, caches: list,
                   rows, q_lens, ctx) -> torch.Tensor:
    """``prefill_extend`` for several sequences of different lengths in
    ONE pass. tokens [T] holds the chunks packed back to back: sequence b
    contributes ``q_lens[b]`` tokens at positions ``ctx[b] ..`` behind the
    ``ctx[b]`` rows the paged caches already hold for it, and uses
    block-table row ``rows[b]`` (``caches`` are the whole-batch caches).
    ``q_lens`` and ``ctx`` are host lists. The per-token ops see a
    [1, T] batch; ``ops.paged_prefill_rope_cache`` appends every token's
    K/V before ``ops.paged_prefill_attention_ragged`` runs, so a sequence
    may read pages another sequence of the same pass fills. Returns the
    logits of each sequence's last token, [B, vocab]."""
    cfg = model.cfg
    rp = RaggedPass.build(model, caches, rows, q_lens, ctx, tokens.device)
    assert tokens.dim() == 1 and tokens.numel() == rp.plan.T
    x = model.embed(tokens[None])
    for blk, cache in zip(model.blocks, caches):
        x = _ragged_attention(model, blk, cache, x, rp)
        xn = ops.rmsnorm(x, blk.mlp_norm, cfg.rms_eps)
        x = x + _mlp_prefill(blk, xn)
    return _ragged_logits(model, x, rp)


@torch.no_grad()
def decode_step(model, token: torch.Tensor, caches: list,
                pos_dev: Optional[torch.Tensor] = None) -> torch.Tensor:
    """One token [B, 1] -> next-position logits [B, vocab], appending to
    the caches. Fully fused decode layer (8 dispatches on GPU): skinny-M
    GEMV x3 + fused GEMV-SwiGLU x1, rope+cache-append x1, split-K
    flash-decode attention x2, fused residual-add+rmsnorm x2. With ``pos_dev`` (int32 device
    scalar) the step is hipGraph-capturable: the cache position comes off
    the device and no host state is read; an int32 [B] ``pos_dev`` runs
    the step RAGGED — every sequence at its own cache position
    (continuous batching, see ContinuousBatcher). ``PagedKVCache``
    caches take the same [B] vector and go through the block-table
    kernels (see PagedBatcher). A Mixtral model runs the same step with
    its active-expert MLP half (``_mlp_decode``), which is
    position-independent; its routing reads the device, so only the
    dense model's step is capturable."""
    cfg = model.cfg
    B = token.shape[0]
    blocks = model.blocks
    paged = isinstance(caches[0], PagedKVCache)
    if paged:
        assert pos_dev is not None and pos_dev.numel() == B, \
            "paged caches need an int32 [B] pos_dev"
        pos = pos_dev
    else:
        pos = caches[0].length if pos_dev is None else pos_dev
    x = model.embed(token).reshape(B, -1)  # [B, H] residual stream
    _, xn = ops.rmsnorm_res(x, None, blocks[0].attn_norm, cfg.rms_eps)
    for i, (blk, cache) in enumerate(zip(blocks, caches)):
        qkv = ops.decode_linear(xn, blk.wqkv.weight)
        if paged:
            q = ops.paged_decode_rope_cache(
                qkv, cache.kpool, cache.vpool, cache.block_table,
                model.rope_cos, model.rope_sin, pos, cfg.num_heads)
            o = ops.paged_decode_attention(q, cache.kpool, cache.vpool,
                                           cache.block_table, pos)
        else:
            q = ops.decode_rope_cache(qkv, cache.k, cache.v, model.rope_cos,
                                      model.rope_sin, pos, cfg.num_heads)
            if pos_dev is None:
                cache.length = pos + 1
                o = ops.decode_attention(q, cache.k, cache.v, pos + 1)
            else:
                # scalar pos_dev: hipGraph loop; [B] pos_dev: ragged decode
                # (continuous batching) — each row attends its own length
                o = ops.decode_attention_dev(q, cache.k, cache.v, pos_dev)
        a = ops.decode_linear(o.reshape(B, -1), blk.wo.weight)
        x, xn = ops.rmsnorm_res(x, a, blk.mlp_norm, cfg.rms_eps)
        m = _mlp_decode(blk, xn)
        w_next = (blocks[i + 1].attn_norm if i + 1 < len(blocks)
                  else model.final_norm)
        x, xn = ops.rmsnorm_res(x, m, w_next, cfg.rms_eps)
    return ops.decode_linear(xn, model.lm_head.weight)


@torch.no_grad()
def generate(
    model,
    tokens: torch.Tensor,
    max_new_tokens: int,
    temperature: float = 0.0,
    top_k: Optional[int] = None,
    max_len: Optional[int] = None,
) -> torch.Tensor:
    """Greedy (temperature=0) or top-k sampled continuation, for a Llama
    or a Mixtral model. tokens [B, S0] -> [B, S0 + max_new_tokens]."""
    cfg = model.cfg
    B, S0 = tokens.shape
    total = S0 + max_new_tokens
    max_len = max_len or total
    assert total <= cfg.max_seq_len, (total, cfg.max_seq_len)
    assert max_len >= total
    device = tokens.device
    caches = [KVCache.empty(cfg, B, max_len, device)
              for _ in range(cfg.num_layers)]

    def pick(logits: torch.Tensor) -> torch.Tensor:
        if temperature <= 0:
            return logits.argmax(-1, keepdim=True)
        logits = logits / temperature
        if top_k:
            kth = torch.topk(logits, top_k, dim=-1).values[:, -1:]
            logits = logits.masked_fill(logits < kth, float("-inf"))
        probs = torch.softmax(logits.float(), dim=-1)
        return torch.multinomial(probs, 1)

    out = [tokens]
    nxt = pick(prefill(model, tokens, caches))
    out.append(nxt)
    for _ in range(max_new_tokens - 1):
        nxt = pick(decode_step(model, nxt, caches))
        out.append(nxt)
    return torch.cat(out, dim=1)


class GraphedDecoder:
    """hipGraph-captured decode loop: the whole per-token step (embed,
    32 layers, lm_head, argmax, cache append, position bump) replays as
    ONE graph with zero host work (the fused eager step is ~260
    dispatches; un-fused it was ~450 and launch-bound). The cache
    length and rope position are driven by a device int32 scalar that
    the captured step increments itself, so one capture serves every
    subsequent token.

    Greedy-only (the argmax feeds back inside the graph).
    """

    def __init__(self, model: LlamaModel, caches: list, batch: int,
                 first_token: torch.Tensor, start_pos: int):
        self.model = model
        self.caches = caches
        cfg = model.cfg
        dev = next(model.parameters()).device
        self.tok = first_token.clone()                      # [B, 1] int64
        self.pos32 = torch.tensor([start_pos], dtype=torch.int32,
                                  device=dev)
        torch.cuda.synchronize()
        self.graph = torch.cuda.CUDAGraph()
        # the eager warmup executes one REAL step (its token is collected
        # in init_tokens); the capture only RECORDS — nothing runs and no
        # state advances during it
        self.init_tokens = []
        self._step_body()                      # eager warm (same code path)
        torch.cuda.synchronize()
        self.init_tokens.append(self.tok.clone())
        with torch.cuda.graph(self.graph):
            self._step_body()
        torch.cuda.synchronize()

    @torch.no_grad()
    def _step_body(self) -> None:
        logits = decode_step(self.model, self.tok, self.caches,
                             pos_dev=self.pos32)
        self.tok.copy_(logits.argmax(-1, keepdim=True))
        self.pos32.add_(1)

    def step(self) -> torch.Tensor:
        """Replay one decode step; returns the new token [B, 1]."""
        self.graph.replay()
        return self.tok


@torch.no_grad()
def generate_graphed(model: LlamaModel, tokens: torch.Tensor,
                     max_new_tokens: int,
                     max_len: Optional[int] = None) -> torch.Tensor:
    """Greedy generation with the hipGraph decode loop (GPU only)."""
    cfg = model.cfg
    B, S0 = tokens.shape
    total = S0 + max_new_tokens
    max_len = max_len or total
    assert total <= cfg.max_seq_len and max_len >= total
    dev = tokens.device
    caches = [KVCache.empty(cfg, B, max_len, dev)
              for _ in range(cfg.num_layers)]
    out = [tokens]
    nxt = prefill(model, tokens, caches).argmax(-1, keepdim=True)
    out.append(nxt)
    if max_new_tokens <= 2:
        for _ in range(max_new_tokens - 1):
            nxt = decode_step(model, nxt, caches).argmax(-1, keepdim=True)
            out.append(nxt)
        return torch.cat(out, dim=1)
    dec = GraphedDecoder(model, caches, B, nxt, start_pos=S0)
    out.extend(t for t in dec.init_tokens[:max_new_tokens - 1])
    remaining = max_new_tokens - 1 - len(dec.init_tokens)
    for _ in range(remaining):
        out.append(dec.step().clone())
    return torch.cat(out, dim=1)


class _Batcher:
    """What the two batchers share: the model, the passes they run and the
    per-row decode state. ``prefill_fn`` / ``decode_fn`` are hooks that
    replace a pass; the defaults serve Llama and Mixtral alike."""

    def __init__(self, model, max_batch: int, max_len: int, prefill_fn,
                 decode_fn):
        self.model = model
        self.cfg = model.cfg
        self._prefill = prefill_fn or prefill
        self._decode = decode_fn or decode_step
        assert max_len <= self.cfg.max_seq_len, "beyond the rope tables"
        dev = next(model.parameters()).device
        self.device = dev
        self.max_len = max_len
        self.pos = torch.zeros(max_batch, dtype=torch.int32, device=dev)
        # host mirror of pos (deterministic: admit sets it, step adds 1) —
        # overflow checks never touch the device
        self.pos_host = [0] * max_batch
        self.tok = torch.zeros(max_batch, 1, dtype=torch.long, device=dev)
        self.active = [False] * max_batch

    def free_rows(self) -> list:
        return [i for i, a in enumerate(self.active) if not a]


class ContinuousBatcher(_Batcher):
    """Continuous batching over a fixed pool of cache rows: sequences of
    DIFFERENT lengths decode together in one ragged step (int32 [B]
    position vector drives rope, cache append and attention per row), and
    a finished row can be re-admitted with a new prompt while the others
    keep decoding — the serving pattern behind vLLM-style engines,
    without paging (288 GB HBM3E holds the whole [B, T] cache pool).

    Greedy decoding; rows are independent — admit() prefills ONE row's
    cache slice, step() advances every active row one token. The model
    may be a Llama or a Mixtral; ``prefill_fn`` / ``decode_fn`` are hooks
    that replace ``prefill`` / ``decode_step``.
    """

    def __init__(self, model, max_batch: int, max_len: int,
                 prefill_fn=None, decode_fn=None):
        super().__init__(model, max_batch, max_len, prefill_fn, decode_fn)
        self.caches = [KVCache.empty(self.cfg, max_batch, max_len,
                                     self.device)
                       for _ in range(self.cfg.num_layers)]

    @torch.no_grad()
    def admit(self, row: int, prompt: torch.Tensor) -> torch.Tensor:
        """Prefill ``prompt`` [S0] into cache row ``row``; returns the
        first generated token (scalar tensor). The row then participates
        in every subsequent step()."""
        assert not self.active[row], f"row {row} is occupied"
        S0 = prompt.numel()
        assert S0 + 1 < self.max_len
        row_caches = [
            KVCache(k=c.k[row:row + 1], v=c.v[row:row + 1], length=0)
            for c in self.caches
        ]
        logits = self._prefill(self.model,
                               prompt.reshape(1, S0).to(self.device),
                               row_caches)
        nxt = logits.argmax(-1)
        self.tok[row, 0] = nxt[0]
        self.pos[row] = S0
        self.pos_host[row] = S0
        self.active[row] = True
        return nxt[0]

    def retire(self, row: int) -> None:
        self.active[row] = False

    @torch.no_grad()
    def step(self) -> torch.Tensor:
        """One ragged decode step over ALL rows (inactive rows compute
        garbage that callers ignore — the batch shape stays static).
        Returns the new tokens [max_batch]."""
        assert any(self.active), "no active sequences"
        logits = self._decode(self.model, self.tok, self.caches,
                              pos_dev=self.pos)
        nxt = logits.argmax(-1, keepdim=True)
        self.tok.copy_(nxt)
        # bound every row (retired rows keep stepping as ignored garbage;
        # the wrap keeps their cache writes in range without a host sync)
        self.pos.add_(1).remainder_(self.max_len)
        for i in range(len(self.pos_host)):
            self.pos_host[i] = (self.pos_host[i] + 1) % self.max_len
            if self.active[i] and self.pos_host[i] + 1 >= self.max_len:
                self.active[i] = False  # out of cache: auto-retire
        return nxt.reshape(-1)


class PagedBatcher(_Batcher):
    """Continuous batching over a PAGED KV pool: same surface as
    ContinuousBatcher (``free_rows``, ``admit``, ``retire``, ``step``),
    but cache memory is committed per ``page_size`` tokens actually
    produced instead of ``max_len`` rows per batch slot. Many short
    requests and a few long ones share ``num_pages`` physical pages per
    layer; a retired row's pages go straight to the next request.

    One int32 [max_batch, M] block table (M = ceil(max_len / page_size))
    is shared by all layers. Physical page 0 is the dump page: a retired
    row's table entries are all 0 and its position is 0 and does not
    advance, so inactive rows read and write only slot 0 of page 0 —
    never pages that may already belong to someone else. When a row
    needs a page and the pool is empty, the row is dropped and its index
    appended to ``self.preempted``.

    ``prefill_chunk=N`` prefills a prompt in pieces of at most N tokens
    through ``prefill_extend``, which bounds the transient activation
    memory of a long prompt.

    ``prefix_sharing=True`` lets a new request map the pages of a live
    row whose prompt starts with the same tokens instead of recomputing
    them. A host-side index maps (parent physical page or -1, the token
    ids of this page) to a physical page, over pages wholly filled by
    PROMPT tokens of live rows; ``admit`` walks the prompt's full pages
    along that chain (at most ``(S0 - 1) // page_size``, so at least one
    token is computed), takes a reference on the hits, allocates the rest
    and prefills from the first uncached position.
    ``self.shared_tokens[row]`` records the hit length. Shared pages are
    never written again — decode appends at positions >= S0, which lie in
    a later page than any indexed one, and a retired row parks on page 0
    — so there is no copy-on-write. A page leaves the index when its last
    holder frees it; a holder of a child page always holds the parent, so
    no stale chain survives a page's reuse. With both options off,
    ``admit`` is the whole-prompt dense-kernel path (``prefill`` on the
    row's caches).

    ``admit_many`` admits several requests in one call and prefills them
    together, packed, through ``prefill_ragged``; it honours both options
    above and leaves the same state as one ``admit`` per request.

    The model may be a Llama or a Mixtral: the passes tell them apart by
    the block. ``prefill_fn``, ``decode_fn``, ``extend_fn`` and
    ``ragged_fn`` are hooks that replace ``prefill``, ``decode_step``,
    ``prefill_extend`` and ``prefill_ragged`` (to count calls, say); no
    model needs them.
    """

    def __init__(self, model, max_batch: int, max_len: int, num_pages: int,
                 page_size: int = 16, prefill_fn=None, decode_fn=None,
                 prefix_sharing: bool = False,
                 prefill_chunk: Optional[int] = None, extend_fn=None,
                 ragged_fn=None):
        super().__init__(model, max_batch, max_len, prefill_fn, decode_fn)
        self._extend = extend_fn or prefill_extend
        self._ragged = ragged_fn or prefill_ragged
        assert prefill_chunk is None or prefill_chunk >= 1
        self.prefix_sharing = prefix_sharing
        self.prefill_chunk = prefill_chunk
        # (parent page or -1, tokens of the page) -> page, and its inverse
        self._index = {}
        self._page_key = {}
        self.shared_tokens = [0] * max_batch
        dev = self.device
        self.page_size = page_size
        self.table_width = -(-max_len // page_size)
        self.block_table = torch.zeros(max_batch, self.table_width,
                                       dtype=torch.int32, device=dev)
        self.caches = [PagedKVCache.empty(self.cfg, num_pages, page_size,
                                          self.block_table, dev)
                       for _ in range(self.cfg.num_layers)]
        self.allocator = PageAllocator(num_pages)
        self.pages = [[] for _ in range(max_batch)]  # pages owned per row
        # 1 for active rows: only those advance (pos.add_(mask))
        self.mask = torch.zeros(max_batch, dtype=torch.int32, device=dev)
        self.preempted = []

    def free_pages(self) -> int:
        return self.allocator.num_free

    @torch.no_grad()
    def admit(self, row: int, prompt: torch.Tensor) -> torch.Tensor:
        """Prefill ``prompt`` [S0] into freshly allocated pages of batch
        row ``row``; returns the first generated token (scalar tensor).
        Raises OutOfPages, with no state changed, when the pool cannot
        hold the prompt plus the first decode position."""
        assert not self.active[row], f"row {row} is occupied"
        S0 = prompt.numel()
        assert S0 + 1 < self.max_len
        if self.prefix_sharing or self.prefill_chunk is not None:
            return self._admit_extend(row, prompt)
        self._set_pages(
            row, self.allocator.alloc(-(-(S0 + 1) // self.page_size)))
        logits = self._prefill(self.model,
                               prompt.reshape(1, S0).to(self.device),
                               [c.for_row(row) for c in self.caches])
        nxt = logits.argmax(-1)
        self._activate([row], nxt, [S0])
        return nxt[0]

    def _admit_extend(self, row: int, prompt: torch.Tensor) -> torch.Tensor:
        """``admit`` through ``extend_fn``: map the cached head of the
        prompt (prefix sharing), prefill the rest in pieces."""
        S0 = prompt.numel()
        # all-or-nothing: _place_prompt allocates before it registers
        # anything, and alloc raises without changing state. The prompt's
        # pages join the index before they are filled; nothing reads the
        # index until the prefill below is done, and this call has no later
        # prompt that could map them.
        hits, pages = self._place_prompt(
            prompt.reshape(-1).tolist(), self._index, self._page_key,
            self.allocator.alloc)
        self.allocator.share(hits)
        self._set_pages(row, pages)
        ctx = len(hits) * self.page_size
        self.shared_tokens[row] = ctx
        piece = self.prefill_chunk or (S0 - ctx)
        row_caches = [c.for_row(row) for c in self.caches]
        prompt_dev = prompt.reshape(1, S0).to(self.device)
        while ctx < S0:
            n = min(piece, S0 - ctx)
            logits = self._extend(self.model, prompt_dev[:, ctx:ctx + n],
                                  row_caches, ctx)
            ctx += n
        nxt = logits.argmax(-1)
        self._activate([row], nxt, [S0])
        return nxt[0]

    def _set_pages(self, row: int, pages: list) -> None:
        self.pages[row] = pages
        self.block_table[row, :len(pages)] = torch.tensor(
            pages, dtype=torch.int32, device=self.device)

    def _activate(self, rows, first: torch.Tensor, lens) -> None:
        """Make ``rows`` live: row ``rows[i]`` holds a prompt of
        ``lens[i]`` tokens and decodes on from ``first[i]``."""
        for i, (row, S0) in enumerate(zip(rows, lens)):
            self.tok[row, 0] = first[i]
            self.pos[row] = S0
            self.mask[row] = 1
            self.pos_host[row] = S0
            self.active[row] = True

    def _count_fresh_pages(self, prompts_toks: list) -> int:
        """Dry run of ``admit_many``'s allocation: the pages the prompts
        need beyond the ones they can map, with prompt j also mapping the
        full pages an earlier prompt of the same call will fill (those
        stand in as negative ids). Changes nothing."""
        # the real placement, over a copy-on-write view of the index and
        # with stand-in page ids (-1 is the root parent)
        staged = ChainMap({}, self._index)
        ids = itertools.count(-2, -1)
        taken = 0

        def stand_ins(n):
            nonlocal taken
            taken += n
            return [next(ids) for _ in range(n)]

        for toks in prompts_toks:
            self._place_prompt(toks, staged, {}, stand_ins)
        return taken

    def _place_prompt(self, toks: list, index, page_key, alloc):
        """Pages for one prompt, as ``admit`` chooses them: map the
        indexed chain over its full pages (at most ``(S0 - 1) // P``, so
        one token is computed), take the rest from ``alloc(n)``, then
        register its own full prompt pages in ``index`` / ``page_key``,
        stopping at a key another row's page already holds. Returns
        (mapped pages, all pages)."""
        P = self.page_size
        S0 = len(toks)
        hits = []
        if self.prefix_sharing:
            parent = -1
            for j in range((S0 - 1) // P):
                page = index.get((parent, tuple(toks[j * P:(j + 1) * P])))
                if page is None:
                    break
                hits.append(page)
                parent = page
        pages = hits + alloc(-(-(S0 + 1) // P) - len(hits))
        if self.prefix_sharing:
            parent = -1
            for j in range(S0 // P):
                key = (parent, tuple(toks[j * P:(j + 1) * P]))
                if index.setdefault(key, pages[j]) != pages[j]:
                    break
                page_key[pages[j]] = key
                parent = pages[j]
        return hits, pages

    @torch.no_grad()
    def admit_many(self, rows, prompts) -> torch.Tensor:
        """``admit`` for several requests at once: prompt i goes to batch
        row ``rows[i]``, and all of them are prefilled together through
        ``ragged_fn`` (packed, each behind its own cached prefix) instead
        of one pass per request. Returns the first generated tokens [n],
        in call order. Raises OutOfPages, with no state changed, unless
        the pool can hold every prompt plus its first decode position.

        With ``prefix_sharing`` the prompts walk and join the index in
        call order, exactly as sequential ``admit`` calls would, so prompt
        j also maps the full pages that prompt i < j of the same call
        fills: every layer appends the K/V of all packed tokens before
        its attention runs. ``prefill_chunk=N`` is a token budget per
        pass: the prompts are packed greedily in call order and split
        across passes where needed, so every token of i is in the same
        or an earlier pass than any token of j > i."""
        rows = [int(r) for r in rows]
        assert len(rows) == len(prompts) >= 1
        assert len(set(rows)) == len(rows), "rows must be distinct"
        P = self.page_size
        toks = [p.reshape(-1).tolist() for p in prompts]
        for row, t in zip(rows, toks):
            assert not self.active[row], f"row {row} is occupied"
            assert 1 <= len(t) and len(t) + 1 < self.max_len
        # all-or-nothing over the whole call, before anything changes
        need = self._count_fresh_pages(toks)
        if need > self.allocator.num_free:
            raise OutOfPages(
                f"need {need} pages, {self.allocator.num_free} free")
        table = torch.zeros(len(rows), self.table_width, dtype=torch.int32)
        starts = []
        for i, (row, t) in enumerate(zip(rows, toks)):
            hits, pages = self._place_prompt(t, self._index, self._page_key,
                                             self.allocator.alloc)
            self.allocator.share(hits)
            self.pages[row] = pages
            table[i, :len(pages)] = torch.tensor(pages, dtype=torch.int32)
            self.shared_tokens[row] = len(hits) * P
            starts.append(len(hits) * P)
        rows_dev = torch.tensor(rows, dtype=torch.long, device=self.device)
        self.block_table[rows_dev] = table.to(self.device)

        # greedy packing in call order under the per-pass token budget
        budget = self.prefill_chunk or sum(len(t) for t in toks)
        passes, cur, room = [], [], budget
        for i, t in enumerate(toks):
            c = starts[i]
            while c < len(t):
                n = min(room, len(t) - c)
                cur.append((i, c, n))
                c += n
                room -= n
                if room == 0:
                    passes.append(cur)
                    cur, room = [], budget
        if cur:
            passes.append(cur)
        prompts_dev = [p.reshape(-1).to(self.device) for p in prompts]
        first = torch.zeros(len(rows), dtype=torch.long, device=self.device)
        for chunk in passes:
            logits = self._ragged(
                self.model,
                torch.cat([prompts_dev[i][c:c + n] for i, c, n in chunk]),
                self.caches, [rows[i] for i, _, _ in chunk],
                [n for _, _, n in chunk], [c for _, c, _ in chunk])
            # sequences whose prompt ends in this pass
            done = [(k, i) for k, (i, c, n) in enumerate(chunk)
                    if c + n == len(toks[i])]
            if done:
                k_dev = torch.tensor([k for k, _ in done], device=self.device)
                i_dev = torch.tensor([i for _, i in done], device=self.device)
                first[i_dev] = logits[k_dev].argmax(-1)
        self._activate(rows, first, [len(t) for t in toks])
        return first

    def retire(self, row: int) -> None:
        """Free the row's pages and park it on the dump page."""
        self.allocator.free(self.pages[row])
        for p in self.pages[row]:
            # last holder gone: the page may be reused, forget its content
            if self.allocator.refcount(p) == 0 and p in self._page_key:
                del self._index[self._page_key.pop(p)]
        self.shared_tokens[row] = 0
        self.pages[row] = []
        self.block_table[row] = 0
        self.pos[row] = 0
        self.mask[row] = 0
        self.pos_host[row] = 0
        self.active[row] = False

    @torch.no_grad()
    def step(self) -> torch.Tensor:
        """One ragged decode step over ALL rows (inactive rows compute
        garbage on the dump page that callers ignore — the batch shape
        stays static). Returns the new tokens [max_batch]; rows dropped
        for lack of pages are listed in ``self.preempted``."""
        assert any(self.active), "no active sequences"
        P = self.page_size
        for i, on in enumerate(self.active):
            # this step appends at pos_host[i]: the row must own that page
            if on and self.pos_host[i] // P >= len(self.pages[i]):
                try:
                    page = self.allocator.alloc(1)[0]
                except OutOfPages:
                    self.retire(i)
                    self.preempted.append(i)
                    continue
                self.block_table[i, len(self.pages[i])] = page
                self.pages[i].append(page)
        logits = self._decode(self.model, self.tok, self.caches,
                              pos_dev=self.pos)
        nxt = logits.argmax(-1, keepdim=True)
        self.tok.copy_(nxt)
        self.pos.add_(self.mask)
        for i, on in enumerate(self.active):
            if on:
                self.pos_host[i] += 1
                if self.pos_host[i] + 1 >= self.max_len:
                    self.retire(i)  # out of cache: auto-retire
        return nxt.reshape(-1)
