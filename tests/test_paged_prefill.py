"""Paged prefill attention over a cached prefix, chunked prefill and
prefix sharing: reference-counted allocator, ``ops.paged_prefill_attention``
(CPU fallback and HIP kernel), ``prefill_extend`` and the PagedBatcher
options.

The HIP kernel keeps the dense forward kernel's tile sequence, MFMA order
and softmax, so for ``ctx % 128 == 0`` the GPU checks ask for bit equality
with ``ops.flash_attention`` on the gathered dense sequence; every case is
also held to the dense forward's bound against an fp32 reference. The CPU
model checks ask for exact equality with whole-prompt ``prefill`` and with
per-sequence greedy generation.
"""

import pytest
import torch

from torchx_amd import ops
from torchx_amd.models.generate import (
    ContinuousBatcher, OutOfPages, PageAllocator, PagedBatcher, PagedKVCache,
    generate, prefill, prefill_extend,
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


# ---------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------


def test_page_allocator_refcounts():
    a = PageAllocator(6)
    x, y, z = a.alloc(3)
    assert [a.refcount(p) for p in (x, y, z)] == [1, 1, 1]
    assert a.refcount(0) == 0
    a.share([x, y])
    a.share([x])
    assert [a.refcount(p) for p in (x, y, z)] == [3, 2, 1]
    assert a.num_free == 2
    a.free([x, y, z])                            # one holder each
    assert [a.refcount(p) for p in (x, y, z)] == [2, 1, 0]
    assert a.num_free == 3                       # only z came back
    assert a.alloc(1) == [z]                     # LIFO
    a.free([y])
    a.free([x])
    assert a.num_free == 3 and a.refcount(x) == 1
    a.free([x])
    # LIFO over last-holder frees: x was freed last
    assert a.alloc(2) == [x, y]
    a.free([x])
    with pytest.raises(AssertionError):
        a.free([x])                              # nobody holds it
    with pytest.raises(AssertionError):
        a.share([x])                             # a free page has no holder
    with pytest.raises(AssertionError):
        a.free([0])


@pytest.mark.parametrize("S", [1, 9, 40])
@pytest.mark.parametrize("ctx_l", [[0, 0, 0], [16, 16, 16], [23, 23, 23],
                                   [0, 16, 23]])
def test_paged_prefill_attention_cpu(ctx_l, S):
    torch.manual_seed(23)
    B, Hq, Hkv, D, P, num_pages = 3, 4, 2, 64, 16, 16
    lengths = [c + S for c in ctx_l]
    bt = _ragged_table(lengths, P, num_pages, seed=3)
    kpool = torch.randn(num_pages, P, Hkv, D).to(torch.bfloat16)
    vpool = torch.randn(num_pages, P, Hkv, D).to(torch.bfloat16)
    q = torch.randn(B, S, Hq, D).to(torch.bfloat16)
    ctx = torch.tensor(ctx_l, dtype=torch.int32)
    o = ops.paged_prefill_attention(q, kpool, vpool, bt, ctx)
    assert o.shape == q.shape and o.dtype == torch.bfloat16
    for b, c in enumerate(ctx_l):
        kd = reference.paged_gather(kpool, bt[b], c + S)
        vd = reference.paged_gather(vpool, bt[b], c + S)
        qfull = torch.zeros(1, c + S, Hq, D, dtype=torch.bfloat16)
        qfull[:, c:] = q[b]
        want = reference.attention(qfull, kd, vd, causal=True)[:, c:]
        assert torch.equal(o[b:b + 1], want), (b, c, S)
        assert torch.equal(
            reference.attention_prefix(q[b:b + 1], kd, vd, c), want)


def _row_caches(cfg, bt, num_pages, P):
    return [PagedKVCache.empty(cfg, num_pages, P, bt, torch.device("cpu"))
            for _ in range(cfg.num_layers)]


@pytest.mark.parametrize("pieces", [(16, 16, 18), (10, 10, 10, 10, 10)])
def test_prefill_extend_pieces_equal_prefill(pieces):
    torch.manual_seed(33)
    cfg = llama_tiny()
    model = LlamaModel(cfg)
    S0, P, num_pages = sum(pieces), 16, 9
    tokens = torch.randint(0, cfg.vocab_size, (1, S0))
    bt = _ragged_table([S0 + 1], P, num_pages, seed=4)
    whole = _row_caches(cfg, bt, num_pages, P)
    want = prefill(model, tokens, [c.for_row(0) for c in whole])
    parts = _row_caches(cfg, bt, num_pages, P)
    ctx = 0
    for n in pieces:
        got = prefill_extend(model, tokens[:, ctx:ctx + n],
                             [c.for_row(0) for c in parts], ctx)
        ctx += n
    assert torch.equal(got, want)
    for cw, cp in zip(whole, parts):
        assert cw.kpool.abs().sum() > 0
        assert torch.equal(cw.kpool, cp.kpool)
        assert torch.equal(cw.vpool, cp.vpool)
    with pytest.raises(AssertionError):          # past the block table
        prefill_extend(model, tokens, [c.for_row(0) for c in parts],
                       bt.shape[1] * P - S0 + 1)


def test_paged_batcher_prefill_chunk_matches_generate():
    torch.manual_seed(43)
    cfg = llama_tiny()
    model = LlamaModel(cfg)
    p1 = torch.randint(0, cfg.vocab_size, (45,))
    p2 = torch.randint(0, cfg.vocab_size, (20,))     # exactly one piece
    solo1 = generate(model, p1.reshape(1, -1), 8)[0, 45:].tolist()
    solo2 = generate(model, p2.reshape(1, -1), 8)[0, 20:].tolist()
    calls = []

    def counting_extend(model, tokens, caches, ctx):
        calls.append((ctx, tokens.shape[1]))
        return prefill_extend(model, tokens, caches, ctx)

    pb = PagedBatcher(model, max_batch=2, max_len=96, num_pages=10,
                      page_size=16, prefill_chunk=20,
                      extend_fn=counting_extend)
    got1, got2 = [int(pb.admit(0, p1))], [int(pb.admit(1, p2))]
    assert calls == [(0, 20), (20, 20), (40, 5), (0, 20)]
    assert pb.shared_tokens == [0, 0]
    for _ in range(7):
        toks = pb.step().tolist()
        got1.append(toks[0])
        got2.append(toks[1])
    assert got1 == solo1, (got1, solo1)
    assert got2 == solo2, (got2, solo2)


def _pools(pb, pages):
    return [(c.kpool[pages].clone(), c.vpool[pages].clone())
            for c in pb.caches]


def test_paged_batcher_prefix_sharing():
    torch.manual_seed(53)
    cfg = llama_tiny()
    model = LlamaModel(cfg)
    head = torch.randint(0, cfg.vocab_size, (40,))
    p0 = torch.cat([head, torch.randint(0, cfg.vocab_size, (9,))])   # 49
    p1 = torch.cat([head, torch.randint(0, cfg.vocab_size, (5,))])   # 45
    solo0 = generate(model, p0.reshape(1, -1), 22)[0, 49:].tolist()
    solo1 = generate(model, p1.reshape(1, -1), 22)[0, 45:].tolist()

    pb = PagedBatcher(model, max_batch=3, max_len=128, num_pages=14,
                      page_size=16, prefix_sharing=True)
    al = pb.allocator
    free0 = pb.free_pages()
    got0 = [int(pb.admit(0, p0))]
    assert pb.shared_tokens[0] == 0
    assert free0 - pb.free_pages() == 4          # ceil(50 / 16)
    shared = pb.pages[0][:2]
    before = _pools(pb, shared)
    free_a = pb.free_pages()
    got1 = [int(pb.admit(1, p1))]
    assert pb.shared_tokens[1] == 32
    assert pb.block_table[1, :2].tolist() == shared
    assert pb.pages[1][:2] == shared
    assert free_a - pb.free_pages() == -(-46 // 16) - 2
    assert [al.refcount(p) for p in shared] == [2, 2]
    for (k0, v0), (k1, v1) in zip(before, _pools(pb, shared)):
        assert torch.equal(k0, k1) and torch.equal(v0, v1)
    for _ in range(9):
        toks = pb.step().tolist()
        got0.append(toks[0])
        got1.append(toks[1])
    assert got0 == solo0[:10], (got0, solo0)
    assert got1 == solo1[:10], (got1, solo1)

    # a 32-token prompt identical to a live row's head shares 1 page: at
    # least one token must be computed
    free_b = pb.free_pages()
    index_b = dict(pb._index)
    pb.admit(2, head[:32])
    assert pb.shared_tokens[2] == 16
    assert pb.pages[2][0] == shared[0] and pb.pages[2][1] != shared[1]
    assert free_b - pb.free_pages() == -(-33 // 16) - 1
    assert pb._index == index_b                  # its 2nd page is a duplicate
    pb.retire(2)
    assert pb.free_pages() == free_b
    assert [al.refcount(p) for p in shared] == [2, 2]

    # row 0 retires: the shared pages stay held, its private ones return
    private0 = pb.pages[0][2:]
    free_c = pb.free_pages()
    pb.retire(0)
    assert pb.free_pages() - free_c == len(private0)
    assert [al.refcount(p) for p in shared] == [1, 1]
    assert all(al.refcount(p) == 0 for p in private0)
    assert pb.block_table[1, :2].tolist() == shared
    for (k0, v0), (k1, v1) in zip(before, _pools(pb, shared)):
        assert torch.equal(k0, k1) and torch.equal(v0, v1)
    for _ in range(6):
        got1.append(pb.step().tolist()[1])
    assert got1 == solo1[:16], (got1, solo1)

    # row 1 retires: everything is back, nothing stays indexed
    pb.retire(1)
    assert pb.free_pages() == free0
    assert pb._index == {} and pb._page_key == {}
    again = [int(pb.admit(0, p1))]
    assert pb.shared_tokens[0] == 0
    for _ in range(15):
        again.append(pb.step().tolist()[0])
    assert again == solo1[:16], (again, solo1)


def test_paged_batcher_prefix_sharing_pressure():
    torch.manual_seed(63)
    cfg = llama_tiny()
    model = LlamaModel(cfg)
    head = torch.randint(0, cfg.vocab_size, (32,))
    p0 = torch.cat([head, torch.randint(0, cfg.vocab_size, (6,))])   # 38
    p1 = torch.cat([head, torch.randint(0, cfg.vocab_size, (40,))])  # 72
    p2 = torch.cat([head, torch.randint(0, cfg.vocab_size, (3,))])   # 35
    solo0 = generate(model, p0.reshape(1, -1), 15)[0, 38:].tolist()
    # 6 usable pages
    pb = PagedBatcher(model, max_batch=3, max_len=96, num_pages=7,
                      page_size=16, prefix_sharing=True)
    al = pb.allocator
    got0 = [int(pb.admit(0, p0))]                # 3 pages
    shared = pb.pages[0][:2]
    # OutOfPages under sharing: p1 needs 5 pages, 2 shared, 3 free
    pb.admit(1, p2)                              # 2 shared + 1 new
    assert pb.free_pages() == 2
    pb.retire(1)
    assert pb.free_pages() == 3
    al.alloc(1)                                  # someone else's page
    table = pb.block_table.clone()
    refs = [al.refcount(p) for p in range(al.num_pages)]
    index = dict(pb._index)
    with pytest.raises(OutOfPages):
        pb.admit(1, p1)                          # needs 3 more, 2 free
    assert torch.equal(pb.block_table, table)
    assert [al.refcount(p) for p in range(al.num_pages)] == refs
    assert pb._index == index and pb.free_rows() == [1, 2]
    assert pb.shared_tokens[1] == 0

    # a sharer that is preempted for lack of pages keeps the other
    # holder's pages alive: row 1 (pos 35) needs a page at pos 48
    pb.admit(1, p2)                              # 2 shared + 1 new: 1 free
    assert pb.free_pages() == 1
    for _ in range(10):                          # row 0 appends at 38..47
        got0.append(pb.step().tolist()[0])
    assert pb.preempted == [] and pb.free_pages() == 1
    got0.append(pb.step().tolist()[0])           # pos 48: the last page
    assert pb.free_pages() == 0 and pb.preempted == []
    for _ in range(2):                           # row 1 appends at 46, 47
        got0.append(pb.step().tolist()[0])
    assert pb.preempted == []
    got0.append(pb.step().tolist()[0])           # row 1 at pos 48: none left
    assert pb.preempted == [1] and pb.active[0]
    assert [al.refcount(p) for p in shared] == [1, 1]
    assert pb.block_table[0, :2].tolist() == shared
    assert got0 == solo0, (got0, solo0)


def test_paged_batcher_mixtral_prefix_sharing_matches_continuous():
    from torchx_amd.models.generate_moe import (
        decode_step_moe, prefill_extend_moe, prefill_moe,
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
                      extend_fn=prefill_extend_moe, **kw)
    want, got = [], []
    for b, out in ((cb, want), (pb, got)):
        out.append([int(b.admit(0, p1)), int(b.admit(1, p2))])
        for _ in range(6):
            out.append(b.step().tolist())
    assert pb.shared_tokens == [0, 16]
    assert got == want, (got, want)


# ---------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------

_KERNEL_CASES = {
    # name: (B, Hq, Hkv, P, ctx, S)
    "xcd_map_partial_tiles": (2, 8, 4, 16, [0, 0], 200),
    "linear_map_ragged_ctx": (3, 4, 2, 16, [0, 128, 256], 70),
    "page_per_tile": (1, 8, 4, 64, [256], 130),
    "tile_inside_page": (1, 4, 2, 256, [256], 130),
    "single_query_row": (1, 4, 2, 16, [384], 1),
    "unaligned_ctx": (2, 8, 4, 16, [77, 5], 100),
    "unaligned_ctx_tiny": (1, 4, 2, 64, [5], 3),
}


def _kernel_inputs(case, dev):
    B, Hq, Hkv, P, ctx_l, S = _KERNEL_CASES[case]
    D = 128
    torch.manual_seed(83)
    lengths = [c + S for c in ctx_l]
    num_pages = sum(-(-L // P) for L in lengths) + 3
    bt = _ragged_table(lengths, P, num_pages, seed=8, device=dev)
    kpool = torch.randn(num_pages, P, Hkv, D, device=dev,
                        dtype=torch.bfloat16)
    vpool = torch.randn(num_pages, P, Hkv, D, device=dev,
                        dtype=torch.bfloat16)
    q = torch.randn(B, S, Hq, D, device=dev, dtype=torch.bfloat16)
    ctx = torch.tensor(ctx_l, dtype=torch.int32, device=dev)
    return q, kpool, vpool, bt, ctx


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(_KERNEL_CASES))
def test_paged_prefill_attention_gpu(case):
    dev = torch.device("cuda:0")
    ctx_l, S = _KERNEL_CASES[case][4:]
    q, kpool, vpool, bt, ctx = _kernel_inputs(case, dev)
    o = ops.paged_prefill_attention(q, kpool, vpool, bt, ctx)
    torch.cuda.synchronize()
    assert o.shape == q.shape
    for b, c in enumerate(ctx_l):
        kd = reference.paged_gather(kpool, bt[b], c + S).contiguous()
        vd = reference.paged_gather(vpool, bt[b], c + S).contiguous()
        ref = reference.attention_prefix(q[b:b + 1].cpu(), kd.cpu(),
                                         vd.cpu(), c)
        err = rel_err(o[b:b + 1].cpu(), ref)
        same = None
        if c % 128 == 0:
            qfull = torch.randn(1, c + S, q.shape[2], 128, device=dev,
                                dtype=torch.bfloat16)
            qfull[:, c:] = q[b]
            dense = ops.flash_attention(qfull, kd, vd, causal=True)[:, c:]
            same = torch.equal(o[b:b + 1], dense)
        print(f"{case}[{b}] ctx={c} S={S}: rel_err vs fp32 {err:.3e}, "
              f"bit-identical to dense: {same}")
        assert same is not False
        assert err < 3e-2, err


@pytest.mark.gpu
def test_paged_prefill_attention_gpu_ignores_table_tail():
    """Entries beyond ceil(L / P) are never used, whatever they hold."""
    dev = torch.device("cuda:0")
    case = "linear_map_ragged_ctx"
    P, ctx_l, S = _KERNEL_CASES[case][3:]
    q, kpool, vpool, bt, ctx = _kernel_inputs(case, dev)
    o = ops.paged_prefill_attention(q, kpool, vpool, bt, ctx)
    bt2 = bt.clone()
    B = len(ctx_l)
    for b, c in enumerate(ctx_l):
        n = -(-(c + S) // P)
        other = bt[(b + 1) % B]                  # another row's valid pages
        bt2[b, n:] = other[:1].expand(bt.shape[1] - n)
    assert not torch.equal(bt, bt2)
    o2 = ops.paged_prefill_attention(q, kpool, vpool, bt2, ctx)
    assert torch.equal(o, o2)


@pytest.mark.gpu
def test_prefill_extend_and_prefix_sharing_gpu():
    from torchx_amd.models.llama import llama_gpu_tiny

    dev = torch.device("cuda:0")
    torch.manual_seed(93)
    cfg = llama_gpu_tiny()
    model = LlamaModel(cfg, device=dev)
    P, num_pages = 16, 24
    tokens = torch.randint(0, cfg.vocab_size, (1, 300), device=dev)
    bt = _ragged_table([301], P, num_pages, seed=9, device=dev)

    def caches():
        return [PagedKVCache.empty(cfg, num_pages, P, bt, dev).for_row(0)
                for _ in range(cfg.num_layers)]

    want = prefill(model, tokens, caches())
    parts, at = caches(), 0
    for n in (128, 128, 44):
        got = prefill_extend(model, tokens[:, at:at + n], parts, at)
        at += n
    err = (got.float() - want.float()).abs().max().item()
    scale = want.float().abs().max().item() + 1e-6
    print(f"prefill_extend (128, 128, 44) vs prefill: max abs err {err:.3e}, "
          f"max |logits| {scale:.3e}")
    assert err < 5e-2 * scale, (err, scale)

    head = torch.randint(0, cfg.vocab_size, (130,), device=dev)
    p0 = torch.cat([head, torch.randint(0, cfg.vocab_size, (20,),
                                        device=dev)])          # 150
    p1 = torch.cat([head, torch.randint(0, cfg.vocab_size, (11,),
                                        device=dev)])          # 141
    pb = PagedBatcher(model, max_batch=2, max_len=256, num_pages=24,
                      page_size=P, prefix_sharing=True)
    al = pb.allocator
    free0 = pb.free_pages()
    pb.admit(0, p0)
    assert pb.shared_tokens[0] == 0
    assert free0 - pb.free_pages() == -(-151 // P)
    shared = pb.pages[0][:8]
    before = _pools(pb, shared)
    free_a = pb.free_pages()
    pb.admit(1, p1)
    assert pb.shared_tokens[1] == 128
    assert pb.block_table[1, :8].tolist() == shared
    assert free_a - pb.free_pages() == -(-142 // P) - 8
    assert [al.refcount(p) for p in shared] == [2] * 8
    for (k0, v0), (k1, v1) in zip(before, _pools(pb, shared)):
        assert torch.equal(k0, k1) and torch.equal(v0, v1)
    for _ in range(10):
        toks = pb.step()
    assert toks.shape == (2,) and pb.preempted == []
    assert pb.pos_host == [160, 151]
    for (k0, v0), (k1, v1) in zip(before, _pools(pb, shared)):
        assert torch.equal(k0, k1) and torch.equal(v0, v1)
    pb.retire(0)
    assert [al.refcount(p) for p in shared] == [1] * 8
    pb.retire(1)
    assert pb.free_pages() == free0
    assert pb._index == {}
