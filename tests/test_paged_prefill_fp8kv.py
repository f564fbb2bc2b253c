"""Paged prefill over fp8 KV pages: ``ops.paged_prefill_attention_fp8kv``
under its fp64 bound over poisoned pools, the ragged form bit for bit
against it, ``ops.paged_prefill_rope_cache_fp8kv`` bit for bit against the
bf16 append + ``ops.quantize_kv_rows``, and
``PagedBatcher(kv_cache="fp8", fp8_prefill=True)``: a batched, prefix-shared
admit against sequential admits."""

import pytest
import torch

from torchx_amd import ops
from torchx_amd.models.generate import PagedBatcher
from torchx_amd.models.llama import LlamaModel, llama_gpu_tiny, llama_tiny
from torchx_amd.ops import bounds as bd

DEV = "cuda:0"

# (id, B, S, Hq, Hkv, P, ctx): the bf16 kernel's cases; G = 8 with a partial
# wave and a partial tile inside one page; G = 1 on the XCD block map
# (B * Hkv = 8) with whole tiles behind ctx % 128 == 0
ATTN_CASES = list(bd.PAGED_CASES) + [
    ("P256-ctx0-S70-g8", 1, 70, 8, 1, 256, [0]),
    ("P32-ctx128,0-S64-g1", 2, 64, 4, 4, 32, [128, 0]),
]


def _poisoned_pools(dense, P, lengths, seed):
    """The logical caches dense = (k8, v8, ks, vs) [B, T, ...] as pools and
    an int32 table [B, M] over seeded pages. Every pool row that holds no
    valid row (page 0, unowned pages, rows at or past lengths[b]) is e4m3
    NaN bytes under a NaN scale and unused table entries are 0, so one read
    outside the valid rows turns the output NaN."""
    B, M = len(lengths), -(-max(lengths) // P) + 1
    g = torch.Generator().manual_seed(seed)
    table = (torch.randperm(B * M, generator=g) + 1).reshape(B, M).to(
        torch.int32).to(DEV)
    pools = []
    for x in dense:
        raw = x.view(torch.uint8) if x.dtype != torch.float32 else x
        fill = float("nan") if x.dtype == torch.float32 else 0x7f
        pool = torch.full((B * M + 1, P) + x.shape[2:], fill, dtype=raw.dtype,
                          device=DEV)
        for b, n in enumerate(lengths):
            t = torch.arange(n, device=DEV)
            pool[table[b, t // P].long(), t % P] = raw[b, :n]
        pools.append(pool.view(x.dtype))
    for b, n in enumerate(lengths):
        table[b, -(-n // P):] = 0
    return pools, table


@pytest.mark.gpu
@pytest.mark.parametrize("family", bd.FAMILIES)
@pytest.mark.parametrize("case", ATTN_CASES, ids=[c[0] for c in ATTN_CASES])
def test_paged_prefill_fp8kv_within_bound(case, family):
    cid, B, S, Hq, Hkv, P, ctx = case
    q, k, v, _ = bd.attention_inputs(family, B, S, Hq, Hkv, T=max(ctx) + S,
                                     seed=bd.case_seed(cid), device=DEV)
    (k8, ks), (v8, vs) = ops.quantize_kv_rows(k), ops.quantize_kv_rows(v)
    ref = bd.prefill_fp8kv_ref_bound(q, k8, v8, ks, vs, bd.SCALE, ctx)
    pools, table = _poisoned_pools((k8, v8, ks, vs), P, [c + S for c in ctx],
                                   bd.case_seed(cid) + 1)
    ctx_t = torch.tensor(ctx, dtype=torch.int32, device=DEV)
    o = ops.paged_prefill_attention_fp8kv(q, *pools, table, ctx_t, bd.SCALE)
    assert o.shape == q.shape and o.dtype == torch.bfloat16
    ratio, ok = bd.bound_ratio(o, ref["o"], ref["o_bound"])
    print(f"paged_prefill_attention_fp8kv {cid} {family}: "
          f"max err/bound {ratio:.3f}")
    assert ok, (cid, family, ratio)


# (Hq, Hkv, q_lens, ctx): 4 tiles x 4 kv heads fill two rounds of 8 units;
# 11 tiles x 1 kv head leave 5 padding units in the second round
RAGGED_CASES = {
    "whole_rounds": (8, 4, (1, 130, 77), (0, 133, 64)),
    "padding_units": (2, 1, (300, 129, 5, 260, 128, 40),
                      (0, 3, 200, 64, 128, 77)),
}


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(RAGGED_CASES))
def test_ragged_fp8kv_equals_each_sequence_alone(case):
    Hq, Hkv, q_lens, ctx = RAGGED_CASES[case]
    B, lengths = len(q_lens), [c + n for c, n in zip(ctx, q_lens)]
    g = torch.Generator().manual_seed(7)
    q = torch.randn(sum(q_lens), Hq, 128, generator=g).bfloat16().to(DEV)
    dense = [y for _ in range(2) for y in ops.quantize_kv_rows(
        torch.randn(B, max(lengths), Hkv, 128, generator=g).to(DEV))]
    pools, table = _poisoned_pools(
        (dense[0], dense[2], dense[1], dense[3]), 16, lengths, 8)
    ctx_t = torch.tensor(ctx, dtype=torch.int32, device=DEV)
    outs = [ops.paged_prefill_attention_ragged_fp8kv(
        q, *pools, table, q_lens, ctx_t, bd.SCALE,
        plan=ops.RaggedPlan(q_lens, DEV, ctx=ctx, heavy_first=heavy))
        for heavy in (False, True)]
    at = 0
    for b, n in enumerate(q_lens):
        alone = ops.paged_prefill_attention_fp8kv(
            q[at:at + n][None], *pools, table[b:b + 1], ctx_t[b:b + 1],
            bd.SCALE)[0]
        assert not alone.isnan().any(), b
        for o in outs:
            assert torch.equal(o[at:at + n], alone), b
        at += n


@pytest.mark.gpu
@pytest.mark.parametrize("P", [16, 64])
def test_ragged_quantising_append_bit_exact(P):
    """Rows with magnitudes spread over 2^+-6, token 0's first k head all
    zero and token 1's first v head with one element 1000 times the rest."""
    Hq, Hkv, q_lens, ctx = 8, 2, (5, 40), (7, 0)
    T, M = sum(q_lens), -(-47 // P)
    g = torch.Generator().manual_seed(3)
    x = torch.randn(T, Hq + 2 * Hkv, 128, generator=g)
    x *= 2.0 ** (torch.rand(T, Hq + 2 * Hkv, 1, generator=g) * 12 - 6)
    x[0, Hq] = 0.0
    x[1, Hq + Hkv, 5] = 1000.0 * x[1, Hq + Hkv].abs().max()
    qkv = x.bfloat16().reshape(T, -1).to(DEV)
    cos, sin = ops.rope_tables(M * P, 128, device=DEV)
    table = (torch.randperm(2 * M, generator=g) + 1).reshape(2, M)
    pos = torch.tensor([c + i for c, n in zip(ctx, q_lens) for i in range(n)])
    seq = torch.tensor([b for b, n in enumerate(q_lens) for _ in range(n)])
    slot = (table[seq, pos // P] * P + pos % P).to(torch.int32).to(DEV)
    pos = pos.to(torch.int32).to(DEV)

    shape = (2 * M + 1, P, Hkv, 128)
    pools16 = [torch.zeros(shape, dtype=torch.bfloat16, device=DEV)
               for _ in range(2)]
    want_q = ops.paged_prefill_rope_cache(qkv, *pools16, cos, sin, pos, slot,
                                          Hq)
    pools = [torch.full(shape, 0.75, device=DEV).to(torch.float8_e4m3fn)
             for _ in range(2)] + [torch.full(shape[:3], 3.0, device=DEV)
                                   for _ in range(2)]
    want = [p.clone() for p in pools]
    got_q = ops.paged_prefill_rope_cache_fp8kv(qkv, *pools, cos, sin, pos,
                                               slot, Hq)
    assert torch.equal(got_q, want_q)
    rows = slot.long()
    for i, pool16 in enumerate(pools16):
        x8, xs = ops.quantize_kv_rows(pool16.view(-1, Hkv, 128)[rows])
        want[i].view(torch.uint8).view(-1, Hkv, 128)[rows] = x8.view(
            torch.uint8)
        want[2 + i].view(-1, Hkv)[rows] = xs
    for name, g_, w in zip(("k8", "v8", "ks", "vs"), pools, want):
        same = torch.equal(g_.view(torch.uint8) if g_.dtype != torch.float32
                           else g_, w.view(torch.uint8)
                           if w.dtype != torch.float32 else w)
        assert same, name


def _state(pb):
    return (pb.block_table.tolist(), pb.pages, pb.shared_tokens, pb._index,
            pb._page_key, pb.allocator._refs, pb.pos_host)


def _pool_bytes(pb):
    return [p.view(torch.uint8) if p.dtype != torch.float32 else p
            for c in pb.caches for p in c.pools]


def _admit_many_equals_sequential(cfg, device, head_len, tails):
    """Row 0 is admitted alone and fills the head's pages; rows 1 and 2 are
    then admitted together (or one by one) and map them."""
    torch.manual_seed(41)
    model = LlamaModel(cfg, device=device)

    def toks(n):
        return torch.randint(0, cfg.vocab_size, (n,), device=device)

    head = toks(head_len)
    prompts = [torch.cat([head, toks(n)]) for n in tails]
    P, npg = 16, head_len // 16
    kw = dict(max_batch=3, max_len=head_len + 64, num_pages=3 * npg + 10,
              page_size=P, kv_cache="fp8", fp8_prefill=True,
              prefix_sharing=True)
    many, seq = PagedBatcher(model, **kw), PagedBatcher(model, **kw)
    chunked = PagedBatcher(model, prefill_chunk=head_len // 2 + 3, **kw)
    first = {}
    for name, pb in (("many", many), ("chunked", chunked)):
        f0 = pb.admit(0, prompts[0])
        shared = pb.pages[0][:npg]
        before = [p[shared].clone() for p in _pool_bytes(pb)]
        assert all(b.float().abs().sum() > 0 for b in before)
        first[name] = [int(f0)] + pb.admit_many([1, 2], prompts[1:]).tolist()
        assert pb.shared_tokens == [0, npg * P, npg * P]
        assert pb.pages[1][:npg] == shared and pb.pages[2][:npg] == shared
        for p, b in zip(_pool_bytes(pb), before):
            assert torch.equal(p[shared], b), name
    first["seq"] = [int(seq.admit(r, p)) for r, p in enumerate(prompts)]
    assert first["many"] == first["seq"]
    assert _state(many) == _state(seq) == _state(chunked)
    for i, (pm, ps) in enumerate(zip(_pool_bytes(many), _pool_bytes(seq))):
        assert torch.equal(pm, ps), f"layer {i // 4} pool {i % 4}"
    for _ in range(4):
        toks_ = many.step()
    assert toks_.shape == (3,) and many.preempted == []
    assert many.pos_host == [len(p) + 4 for p in prompts]


@pytest.mark.gpu
def test_fp8_admit_many_equals_sequential_admits_gpu():
    _admit_many_equals_sequential(llama_gpu_tiny(), DEV, 128, (20, 11, 3))


def test_fp8_admit_many_equals_sequential_admits_cpu():
    _admit_many_equals_sequential(llama_tiny(), "cpu", 32, (9, 5, 7))
