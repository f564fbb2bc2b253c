"""Batched admit for the paged batcher: ``ops.paged_prefill_attention_ragged``
and ``ops.paged_prefill_rope_cache`` (CPU fallbacks and HIP kernels),
``prefill_ragged`` / ``prefill_ragged_moe`` and ``PagedBatcher.admit_many``.

The ragged attention kernel runs, per (sequence, q tile, head), the block
work of ``paged_prefill_attn_kernel`` on that sequence alone, and the append
kernel uses the rope kernel's rotation expression, so the GPU checks ask
for bit equality with the existing ops, not a tolerance. The CPU model
checks ask for equality with sequential ``admit`` and per-sequence greedy
generation.
"""

import pytest
import torch

from torchx_amd import ops
from torchx_amd.models.generate import (
    ContinuousBatcher, OutOfPages, PagedBatcher, PagedKVCache, generate,
    prefill_extend, prefill_ragged,
)
from torchx_amd.models.llama import LlamaModel, llama_tiny
from torchx_amd.ops import reference


def rel_err(a, b):
    a, b = a.float(), b.float()
    return (a - b).abs().max().item() / (b.abs().max().item() + 1e-6)


def _ragged_table(lengths, P, num_pages, seed, extra=2, device="cpu"):
    """int32 [B, M]: row b's first ceil(lengths[b] / P) entries are
    distinct physical pages from a seeded permutation of 1..num_pages-1;
    the unused entries stay 0."""
    n = [-(-L // P) for L in lengths]
    assert sum(n) <= num_pages - 1
    g = torch.Generator().manual_seed(seed)
    perm = (torch.randperm(num_pages - 1, generator=g) + 1).to(torch.int32)
    bt = torch.zeros(len(lengths), max(n) + extra, dtype=torch.int32)
    at = 0
    for b, nb in enumerate(n):
        bt[b, :nb] = perm[at:at + nb]
        at += nb
    return bt.to(device)


def _cu(q_lens):
    cu = [0]
    for n in q_lens:
        cu.append(cu[-1] + n)
    return cu


def _attn_inputs(Hq, Hkv, D, P, q_lens, ctx_l, dev, seed):
    torch.manual_seed(seed)
    lengths = [c + n for c, n in zip(ctx_l, q_lens)]
    num_pages = sum(-(-L // P) for L in lengths) + 3
    bt = _ragged_table(lengths, P, num_pages, seed=seed, device=dev)
    kpool = torch.randn(num_pages, P, Hkv, D, device=dev,
                        dtype=torch.bfloat16)
    vpool = torch.randn(num_pages, P, Hkv, D, device=dev,
                        dtype=torch.bfloat16)
    q = torch.randn(sum(q_lens), Hq, D, device=dev, dtype=torch.bfloat16)
    ctx = torch.tensor(ctx_l, dtype=torch.int32, device=dev)
    return q, kpool, vpool, bt, ctx


def _rope_tables(rows, D, dev):
    inv = 1.0 / (10000.0 ** (torch.arange(0, D, 2).float() / D))
    ang = torch.arange(rows).float()[:, None] * inv[None]
    return ang.cos().to(dev), ang.sin().to(dev)


def _pos_slot(bt, P, q_lens, ctx_l, dev):
    pos = [c + i for c, n in zip(ctx_l, q_lens) for i in range(n)]
    seq = [b for b, n in enumerate(q_lens) for _ in range(n)]
    slot = [int(bt[b, p // P]) * P + p % P for b, p in zip(seq, pos)]
    return (torch.tensor(pos, dtype=torch.int32, device=dev),
            torch.tensor(slot, dtype=torch.int32, device=dev))


def _check_rope_cache(Hq, Hkv, D, P, q_lens, ctx_l, dev, seed):
    """q and both pools equal ``ops.rope`` + ``store_rows`` per sequence;
    pool rows not named in ``slot`` keep their content."""
    torch.manual_seed(seed)
    lengths = [c + n for c, n in zip(ctx_l, q_lens)]
    num_pages = sum(-(-L // P) for L in lengths) + 3
    bt = _ragged_table(lengths, P, num_pages, seed=seed, device=dev)
    T = sum(q_lens)
    qkv = torch.randn(T, (Hq + 2 * Hkv) * D, device=dev,
                      dtype=torch.bfloat16)
    cos, sin = _rope_tables(max(lengths) + 5, D, dev)
    kpool = torch.randn(num_pages, P, Hkv, D, device=dev,
                        dtype=torch.bfloat16)
    vpool = torch.randn_like(kpool)
    k0, v0 = kpool.clone(), vpool.clone()
    kref, vref = kpool.clone(), vpool.clone()
    pos, slot = _pos_slot(bt.cpu(), P, q_lens, ctx_l, dev)

    q = ops.paged_prefill_rope_cache(qkv, kpool, vpool, cos, sin, pos, slot,
                                     Hq)
    assert q.shape == (T, Hq, D) and q.is_contiguous()

    cu = _cu(q_lens)
    for b, (c, n) in enumerate(zip(ctx_l, q_lens)):
        part = qkv[cu[b]:cu[b + 1]]
        qb, kb, vb = part.split([Hq * D, Hkv * D, Hkv * D], dim=-1)
        cs, sn = cos[c:c + n], sin[c:c + n]
        want_q = ops.rope(qb.reshape(1, n, Hq, D).contiguous(), cs, sn)
        want_k = ops.rope(kb.reshape(1, n, Hkv, D).contiguous(), cs, sn)
        PagedKVCache(kref, vref, bt, row=b).store_rows(
            want_k, vb.reshape(1, n, Hkv, D).contiguous(), c)
        assert torch.equal(q[cu[b]:cu[b + 1]], want_q[0]), b
    assert torch.equal(kpool, kref) and torch.equal(vpool, vref)
    keep = torch.ones(num_pages * P, dtype=torch.bool, device=dev)
    keep[slot.long()] = False
    assert int(keep.sum()) == num_pages * P - T
    for pool, before in ((kpool, k0), (vpool, v0)):
        assert torch.equal(pool.view(-1, Hkv, D)[keep],
                           before.view(-1, Hkv, D)[keep])
        assert not torch.equal(pool, before)


# ---------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("q_lens,ctx_l", [([9, 1, 40], [0, 16, 23]),
                                          ([1, 1, 1], [5, 0, 31])])
def test_paged_prefill_attention_ragged_cpu(q_lens, ctx_l):
    q, kpool, vpool, bt, ctx = _attn_inputs(4, 2, 64, 16, q_lens, ctx_l,
                                            "cpu", seed=13)
    o = ops.paged_prefill_attention_ragged(q, kpool, vpool, bt, q_lens, ctx)
    assert o.shape == q.shape and o.dtype == torch.bfloat16
    plan = ops.RaggedPlan(q_lens, q.device, ctx=ctx_l)
    assert plan.cu == _cu(q_lens) and plan.T == sum(q_lens)
    o2 = ops.paged_prefill_attention_ragged(q, kpool, vpool, bt, q_lens, ctx,
                                            plan=plan)
    assert torch.equal(o, o2)
    cu = _cu(q_lens)
    for b in range(len(q_lens)):
        want = ops.paged_prefill_attention(
            q[cu[b]:cu[b + 1]][None], kpool, vpool, bt[b:b + 1],
            ctx[b:b + 1])
        assert torch.equal(o[cu[b]:cu[b + 1]], want[0]), b


def test_ragged_plan_tiles():
    q_lens, ctx_l = [130, 1, 128, 70], [0, 384, 128, 77]
    flat = ops.RaggedPlan(q_lens, "cpu", ctx=ctx_l, heavy_first=False)
    assert flat.tiles_host == [(0, 0, 0, 130), (0, 1, 0, 130),
                               (1, 0, 130, 1), (2, 0, 131, 128),
                               (3, 0, 259, 70)]
    assert flat.tiles.dtype == torch.int32 and flat.tiles.shape == (5, 4)
    heavy = ops.RaggedPlan(q_lens, "cpu", ctx=ctx_l, heavy_first=True)
    # keys attended: 128, 130, 385, 256, 147
    assert heavy.tiles_host == [(1, 0, 130, 1), (2, 0, 131, 128),
                                (3, 0, 259, 70), (0, 1, 0, 130),
                                (0, 0, 0, 130)]
    assert sorted(heavy.tiles_host) == sorted(flat.tiles_host)
    with pytest.raises(AssertionError):
        ops.RaggedPlan([3, 0], "cpu")


def test_paged_prefill_rope_cache_cpu():
    _check_rope_cache(4, 2, 64, 16, [9, 1, 40], [0, 16, 23], "cpu", seed=14)


_PROMPT_LENS = (45, 20, 33, 1)


def _tiny_model_and_prompts(seed):
    torch.manual_seed(seed)
    cfg = llama_tiny()
    model = LlamaModel(cfg)
    prompts = [torch.randint(0, cfg.vocab_size, (n,)) for n in _PROMPT_LENS]
    return model, prompts


@pytest.fixture(scope="module")
def tiny103():
    """llama_tiny, the four prompts and their solo greedy continuations
    (8 tokens each), computed once for the admit_many tests."""
    model, prompts = _tiny_model_and_prompts(103)
    solo = [generate(model, p.reshape(1, -1), 8)[0, p.numel():].tolist()
            for p in prompts]
    return model, prompts, solo


def _run_steps(pb, first, rows, steps):
    got = [[int(t)] for t in first]
    for _ in range(steps):
        toks = pb.step().tolist()
        for g, r in zip(got, rows):
            g.append(toks[r])
    return got


def test_admit_many_matches_sequential_admit_and_generate(tiny103):
    model, prompts, solo = tiny103
    kw = dict(max_batch=4, max_len=96, num_pages=16, page_size=16)
    many, seq = PagedBatcher(model, **kw), PagedBatcher(model, **kw)
    first = many.admit_many([0, 1, 2, 3], prompts)
    assert first.shape == (4,)
    first_seq = [int(seq.admit(r, p)) for r, p in enumerate(prompts)]
    assert first.tolist() == first_seq
    assert torch.equal(many.block_table, seq.block_table)
    assert many.pages == seq.pages and many.pos_host == seq.pos_host
    assert torch.equal(many.pos, seq.pos) and torch.equal(many.mask, seq.mask)
    assert torch.equal(many.tok, seq.tok) and many.active == seq.active
    for cm, cs in zip(many.caches, seq.caches):
        assert cm.kpool.abs().sum() > 0
        assert torch.equal(cm.kpool, cs.kpool)
        assert torch.equal(cm.vpool, cs.vpool)
    got = _run_steps(many, first, range(4), 7)
    assert got == solo, (got, solo)
    with pytest.raises(AssertionError):
        many.admit_many([0], prompts[:1])            # row 0 is occupied
    with pytest.raises(AssertionError):
        PagedBatcher(model, **kw).admit_many([1, 1], prompts[:2])


def test_admit_many_prefill_chunk_packs_greedily(tiny103):
    model, prompts, solo = tiny103
    calls = []

    def counting_ragged(model, tokens, caches, rows, q_lens, ctx):
        calls.append((list(rows), list(q_lens), list(ctx)))
        return prefill_ragged(model, tokens, caches, rows, q_lens, ctx)

    pb = PagedBatcher(model, max_batch=5, max_len=96, num_pages=16,
                      page_size=16, prefill_chunk=32,
                      ragged_fn=counting_ragged)
    rows = [4, 0, 2, 1]
    first = pb.admit_many(rows, prompts)
    # 45 / 20 / 33 / 1 tokens under a budget of 32 per pass
    assert calls == [([4], [32], [0]),
                     ([4, 0], [13, 19], [32, 0]),
                     ([0, 2], [1, 31], [19, 0]),
                     ([2, 1], [2, 1], [31, 0])]
    assert pb.free_rows() == [3] and pb.shared_tokens == [0] * 5
    got = _run_steps(pb, first, rows, 7)
    assert got == solo, (got, solo)


def test_admit_many_prefix_sharing():
    torch.manual_seed(53)
    cfg = llama_tiny()
    model = LlamaModel(cfg)
    head = torch.randint(0, cfg.vocab_size, (40,))
    tails = [torch.randint(0, cfg.vocab_size, (n,)) for n in (9, 5, 7)]
    p9, p5, p7 = [torch.cat([head, t]) for t in tails]
    solo = {n: generate(model, p.reshape(1, -1), 8)[0, p.numel():].tolist()
            for n, p in ((9, p9), (5, p5), (7, p7))}
    kw = dict(max_batch=3, max_len=128, num_pages=14, page_size=16,
              prefix_sharing=True)

    # across live rows: row 0 holds the head's two full pages
    pb = PagedBatcher(model, **kw)
    seq = PagedBatcher(model, **kw)
    al = pb.allocator
    free0 = pb.free_pages()
    f0 = pb.admit(0, p9)
    shared = pb.pages[0][:2]
    first = pb.admit_many([1, 2], [p5, p7])
    assert pb.shared_tokens[1:] == [32, 32]
    assert pb.pages[1][:2] == shared and pb.pages[2][:2] == shared
    assert pb.block_table[1, :2].tolist() == shared
    assert pb.block_table[2, :2].tolist() == shared
    assert [al.refcount(p) for p in shared] == [3, 3]
    # exactly the state three sequential admits leave
    for r, p in enumerate((p9, p5, p7)):
        seq.admit(r, p)
    assert pb.pages == seq.pages and pb.shared_tokens == seq.shared_tokens
    assert pb._index == seq._index and pb._page_key == seq._page_key
    assert al._refs == seq.allocator._refs
    assert torch.equal(pb.block_table, seq.block_table)
    got = _run_steps(pb, [f0] + list(first), range(3), 7)
    assert got == [solo[9], solo[5], solo[7]], got
    for r in range(3):
        pb.retire(r)
    assert pb.free_pages() == free0
    assert pb._index == {} and pb._page_key == {}

    # inside one call: prompt 1 maps the pages prompt 0 fills
    pb = PagedBatcher(model, **kw)
    seq = PagedBatcher(model, **kw)
    al = pb.allocator
    first = pb.admit_many([0, 1], [p9, p5])
    assert pb.shared_tokens[:2] == [0, 32]
    shared = pb.pages[0][:2]
    assert pb.pages[1][:2] == shared
    assert [al.refcount(p) for p in shared] == [2, 2]
    assert free0 - pb.free_pages() == -(-50 // 16) + -(-46 // 16) - 2
    for r, p in enumerate((p9, p5)):
        seq.admit(r, p)
    assert pb.pages == seq.pages and pb._index == seq._index
    assert pb._page_key == seq._page_key
    assert al._refs == seq.allocator._refs
    for cm, cs in zip(pb.caches, seq.caches):
        assert torch.equal(cm.kpool, cs.kpool)
        assert torch.equal(cm.vpool, cs.vpool)
    got = _run_steps(pb, first, range(2), 7)
    assert got == [solo[9], solo[5]], got
    pb.retire(0)
    pb.retire(1)
    assert pb.free_pages() == free0
    assert pb._index == {} and pb._page_key == {}


def test_admit_many_out_of_pages_changes_nothing():
    torch.manual_seed(63)
    cfg = llama_tiny()
    model = LlamaModel(cfg)
    head = torch.randint(0, cfg.vocab_size, (32,))
    p0 = torch.cat([head, torch.randint(0, cfg.vocab_size, (6,))])    # 38
    pa = torch.cat([head, torch.randint(0, cfg.vocab_size, (3,))])    # 35
    pbig = torch.cat([head, torch.randint(0, cfg.vocab_size, (40,))])  # 72
    # 6 usable pages, row 0 holds 3
    pb = PagedBatcher(model, max_batch=3, max_len=96, num_pages=7,
                      page_size=16, prefix_sharing=True)
    al = pb.allocator
    pb.admit(0, p0)
    assert pb.free_pages() == 3
    table = pb.block_table.clone()
    refs = list(al._refs)
    index, page_key = dict(pb._index), dict(pb._page_key)
    pools = [(c.kpool.clone(), c.vpool.clone()) for c in pb.caches]
    # the first prompt fits (2 shared + 1 new), the second needs 3 more
    with pytest.raises(OutOfPages):
        pb.admit_many([1, 2], [pa, pbig])
    assert torch.equal(pb.block_table, table)
    assert al._refs == refs and pb.free_pages() == 3
    assert pb._index == index and pb._page_key == page_key
    assert pb.free_rows() == [1, 2] and pb.shared_tokens == [0, 0, 0]
    assert pb.pages[1] == [] and pb.pages[2] == []
    for c, (k, v) in zip(pb.caches, pools):
        assert torch.equal(c.kpool, k) and torch.equal(c.vpool, v)
    # and the same call goes through once it fits: 3 + 3 pages, 6 free
    pb.retire(0)
    assert pb.free_pages() == 6
    pb.admit_many([1, 2], [pa, pbig])
    assert pb.shared_tokens == [0, 0, 32] and pb.free_pages() == 0


def test_admit_many_mixtral_matches_continuous():
    from torchx_amd.models.generate_moe import (
        decode_step_moe, prefill_extend_moe, prefill_moe, prefill_ragged_moe,
    )
    from torchx_amd.models.mixtral import MixtralModel, mixtral_tiny

    torch.manual_seed(73)
    cfg = mixtral_tiny()
    model = MixtralModel(cfg)
    head = torch.randint(0, cfg.vocab_size, (20,))
    p1 = torch.cat([head, torch.randint(0, cfg.vocab_size, (3,))])
    p2 = torch.cat([head, torch.randint(0, cfg.vocab_size, (10,))])
    kw = dict(prefill_fn=prefill_moe, decode_fn=decode_step_moe)
    cb = ContinuousBatcher(model, max_batch=2, max_len=64, **kw)
    pb = PagedBatcher(model, max_batch=2, max_len=64, num_pages=8,
                      page_size=16, prefix_sharing=True,
                      extend_fn=prefill_extend_moe,
                      ragged_fn=prefill_ragged_moe, **kw)
    want = [[int(cb.admit(0, p1)), int(cb.admit(1, p2))]]
    got = [pb.admit_many([0, 1], [p1, p2]).tolist()]
    for _ in range(6):
        want.append(cb.step().tolist())
        got.append(pb.step().tolist())
    assert pb.shared_tokens == [0, 16]
    assert got == want, (got, want)


# ---------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------

_RAGGED_CASES = {
    # name: (Hq, Hkv, P, q_lens, ctx)
    "mixed": (8, 4, 16, [130, 1, 128, 70], [0, 384, 128, 77]),
    "single_sequence": (4, 2, 64, [200], [256]),
    "decode_like": (4, 2, 16, [1, 1, 1], [5, 130, 0]),
    "tile_inside_page": (4, 2, 256, [3, 260], [5, 256]),
    # the block map with G = 2 and no padding units (tiles * Hkv a multiple
    # of 8), two tiles per sequence, unaligned ctx
    "no_padding_units": (8, 4, 16, [129, 200], [3, 64]),
    # Hkv = 8: every tile of a kv head on one XCD
    "hkv8": (16, 8, 16, [140, 20], [10, 300]),
}


def test_ragged_cases_cover_both_sides_of_the_block_map():
    """The grid is rounded up to rounds of 8 (tile, kv head) units: some
    cases must have padding units that leave early, some none."""
    padded = {name: (sum(-(-n // 128) for n in c[3]) * c[1]) % 8 != 0
              for name, c in _RAGGED_CASES.items()}
    assert padded["mixed"] and padded["single_sequence"]
    assert not padded["no_padding_units"] and not padded["hkv8"]


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(_RAGGED_CASES))
def test_paged_prefill_attention_ragged_gpu(case):
    dev = torch.device("cuda:0")
    Hq, Hkv, P, q_lens, ctx_l = _RAGGED_CASES[case]
    q, kpool, vpool, bt, ctx = _attn_inputs(Hq, Hkv, 128, P, q_lens, ctx_l,
                                            dev, seed=83)
    o = ops.paged_prefill_attention_ragged(q, kpool, vpool, bt, q_lens, ctx)
    # the tile order is a scheduling choice only
    for heavy in (False, True):
        plan = ops.RaggedPlan(q_lens, dev, ctx=ctx_l, heavy_first=heavy)
        o2 = ops.paged_prefill_attention_ragged(q, kpool, vpool, bt, q_lens,
                                                ctx, plan=plan)
        assert torch.equal(o, o2), heavy
    torch.cuda.synchronize()
    assert o.shape == q.shape
    cu = _cu(q_lens)
    for b, (c, n) in enumerate(zip(ctx_l, q_lens)):
        qb = q[cu[b]:cu[b + 1]][None].contiguous()
        alone = ops.paged_prefill_attention(qb, kpool, vpool, bt[b:b + 1],
                                            ctx[b:b + 1])
        same = torch.equal(o[cu[b]:cu[b + 1]], alone[0])
        kd = reference.paged_gather(kpool, bt[b], c + n).cpu()
        vd = reference.paged_gather(vpool, bt[b], c + n).cpu()
        ref = reference.attention_prefix(qb.cpu(), kd, vd, c)
        err = rel_err(o[cu[b]:cu[b + 1]].cpu(), ref[0])
        print(f"{case}[{b}] ctx={c} n={n}: bit-identical to the sequence "
              f"alone: {same}, rel_err vs fp32 {err:.3e}")
        assert same
        assert err < 3e-2, err


@pytest.mark.gpu
def test_paged_prefill_attention_ragged_gpu_isolation():
    """A sequence's output depends on nothing of another sequence: not its
    q rows, not its private pages, not the table beyond ceil(L / P)."""
    dev = torch.device("cuda:0")
    Hq, Hkv, P, q_lens, ctx_l = _RAGGED_CASES["mixed"]
    q, kpool, vpool, bt, ctx = _attn_inputs(Hq, Hkv, 128, P, q_lens, ctx_l,
                                            dev, seed=84)
    o = ops.paged_prefill_attention_ragged(q, kpool, vpool, bt, q_lens, ctx)
    cu = _cu(q_lens)
    B = len(q_lens)
    npages = [-(-(c + n) // P) for c, n in zip(ctx_l, q_lens)]
    for victim in range(B):
        q2, k2, v2, bt2 = q.clone(), kpool.clone(), vpool.clone(), bt.clone()
        q2[cu[victim]:cu[victim + 1]] = 7.0
        own = bt[victim, :npages[victim]].long()
        k2[own] = -3.0
        v2[own] = 5.0
        for b in range(B):                       # table tails: valid pages
            bt2[b, npages[b]:] = bt[victim, 0]
        assert not torch.equal(bt, bt2)
        o2 = ops.paged_prefill_attention_ragged(q2, k2, v2, bt2, q_lens, ctx)
        for b in range(B):
            same = torch.equal(o[cu[b]:cu[b + 1]], o2[cu[b]:cu[b + 1]])
            assert same == (b != victim), (victim, b)


@pytest.mark.gpu
@pytest.mark.parametrize("q_lens,ctx_l", [([130, 1, 128, 70],
                                           [0, 384, 128, 77]),
                                          ([1], [37])])
def test_paged_prefill_rope_cache_gpu(q_lens, ctx_l):
    _check_rope_cache(8, 4, 128, 16, q_lens, ctx_l, torch.device("cuda:0"),
                      seed=85)


def _loop_attention(q, kpool, vpool, block_table, q_lens, ctx, scale=None,
                    plan=None):
    """The ragged op as a loop of the existing op per sequence."""
    cu = _cu(q_lens)
    return torch.cat([
        ops.paged_prefill_attention(q[cu[b]:cu[b + 1]][None].contiguous(),
                                    kpool, vpool, block_table[b:b + 1],
                                    ctx[b:b + 1], scale)[0]
        for b in range(len(q_lens))])


def _unfused_rope_cache(qkv, kpool, vpool, cos, sin, pos, slot, num_heads):
    """The fused append as the dispatches it replaces: split, contiguous
    copies, two ropes, one index_copy_ per pool (what store_rows does)."""
    T = qkv.shape[0]
    Hkv, D = kpool.shape[2], kpool.shape[3]
    q, k, v = qkv.split([num_heads * D, Hkv * D, Hkv * D], dim=-1)
    cs, sn = cos[pos.long()], sin[pos.long()]
    q = ops.rope(q.reshape(1, T, num_heads, D).contiguous(), cs, sn)
    k = ops.rope(k.reshape(1, T, Hkv, D).contiguous(), cs, sn)
    kpool.view(-1, Hkv, D).index_copy_(0, slot.long(), k[0])
    vpool.view(-1, Hkv, D).index_copy_(
        0, slot.long(), v.reshape(T, Hkv, D).contiguous())
    return q[0]


@pytest.mark.gpu
def test_prefill_ragged_gpu(monkeypatch):
    from torchx_amd.models.llama import llama_gpu_tiny

    dev = torch.device("cuda:0")
    torch.manual_seed(93)
    cfg = llama_gpu_tiny()
    model = LlamaModel(cfg, device=dev)
    P, num_pages = 16, 28
    q_lens, ctx_l = [130, 1, 70], [0, 128, 16]
    lengths = [c + n for c, n in zip(ctx_l, q_lens)]
    seqs = [torch.randint(0, cfg.vocab_size, (L,), device=dev)
            for L in lengths]
    bt = _ragged_table([L + 1 for L in lengths], P, num_pages, seed=9,
                       device=dev)
    packed = torch.cat([s[c:] for s, c in zip(seqs, ctx_l)])

    def caches_with_prefixes():
        caches = [PagedKVCache.empty(cfg, num_pages, P, bt, dev)
                  for _ in range(cfg.num_layers)]
        for b, c in enumerate(ctx_l):
            if c:
                prefill_extend(model, seqs[b][None, :c],
                               [x.for_row(b) for x in caches], 0)
        return caches

    fused = caches_with_prefixes()
    got = prefill_ragged(model, packed, fused, [0, 1, 2], q_lens, ctx_l)
    assert got.shape == (3, cfg.vocab_size)

    # only the two kernels differ from per-sequence loops: exact
    loops = caches_with_prefixes()
    with monkeypatch.context() as m:
        m.setattr(ops, "paged_prefill_attention_ragged", _loop_attention)
        m.setattr(ops, "paged_prefill_rope_cache", _unfused_rope_cache)
        want = prefill_ragged(model, packed, loops, [0, 1, 2], q_lens, ctx_l)
    assert torch.equal(got, want)
    for cf, cl in zip(fused, loops):
        assert cf.kpool.abs().sum() > 0
        assert torch.equal(cf.kpool, cl.kpool)
        assert torch.equal(cf.vpool, cl.vpool)

    # against prefill_extend per sequence: other GEMM row counts
    solo = caches_with_prefixes()
    for b, c in enumerate(ctx_l):
        ref = prefill_extend(model, seqs[b][None, c:],
                             [x.for_row(b) for x in solo], c)
        err = (got[b].float() - ref[0].float()).abs().max().item()
        scale = ref.float().abs().max().item() + 1e-6
        print(f"prefill_ragged seq {b} (n={q_lens[b]}, ctx={c}) vs "
              f"prefill_extend: max abs err {err:.3e}, max |logits| "
              f"{scale:.3e}")
        assert err < 5e-2 * scale, (b, err, scale)


@pytest.mark.gpu
def test_admit_many_gpu():
    from torchx_amd.models.llama import llama_gpu_tiny

    dev = torch.device("cuda:0")
    torch.manual_seed(94)
    cfg = llama_gpu_tiny()
    model = LlamaModel(cfg, device=dev)
    P = 16
    head = torch.randint(0, cfg.vocab_size, (130,), device=dev)
    p0 = torch.cat([head, torch.randint(0, cfg.vocab_size, (20,),
                                        device=dev)])          # 150
    p1 = torch.cat([head, torch.randint(0, cfg.vocab_size, (11,),
                                        device=dev)])          # 141
    p2 = torch.randint(0, cfg.vocab_size, (20,), device=dev)
    pb = PagedBatcher(model, max_batch=3, max_len=256, num_pages=32,
                      page_size=P, prefix_sharing=True)
    al = pb.allocator
    free0 = pb.free_pages()
    first = pb.admit_many([0, 1, 2], [p0, p1, p2])
    assert first.shape == (3,)
    assert pb.shared_tokens == [0, 128, 0]
    shared = pb.pages[0][:8]
    assert pb.block_table[1, :8].tolist() == shared
    assert free0 - pb.free_pages() == \
        -(-151 // P) + -(-142 // P) - 8 + -(-21 // P)
    assert [al.refcount(p) for p in shared] == [2] * 8
    assert torch.equal(pb.tok[:, 0], first)
    before = [(c.kpool[shared].clone(), c.vpool[shared].clone())
              for c in pb.caches]
    assert all(k.abs().sum() > 0 for k, _ in before)
    for _ in range(10):
        toks = pb.step()
    assert toks.shape == (3,) and pb.preempted == []
    assert pb.pos_host == [160, 151, 30]
    assert pb.pos.tolist() == [160, 151, 30]
    assert [al.refcount(p) for p in shared] == [2] * 8
    for c, (k, v) in zip(pb.caches, before):
        assert torch.equal(c.kpool[shared], k)
        assert torch.equal(c.vpool[shared], v)
    pb.retire(0)
    assert [al.refcount(p) for p in shared] == [1] * 8
    pb.retire(1)
    pb.retire(2)
    assert pb.free_pages() == free0
    assert pb._index == {} and pb._page_key == {}
