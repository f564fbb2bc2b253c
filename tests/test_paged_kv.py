"""Paged KV cache: page allocator, block-table decode ops (CPU fallback
and HIP kernels), PagedBatcher.

The paged kernels keep the dense kernels' row-to-lane assignment, split
boundaries and arithmetic order, so the GPU checks ask for bit equality
with the dense path on the same logical cache, and the batcher checks ask
for exact token equality with per-sequence greedy generation.
"""

import pytest
import torch

from torchx_amd import ops
from torchx_amd.models.generate import (
    ContinuousBatcher, OutOfPages, PageAllocator, PagedBatcher, generate,
)
from torchx_amd.models.llama import LlamaModel, llama_tiny
from torchx_amd.ops import reference


def _shuffled_table(B, pages_per_row, M, num_pages, seed, device="cpu"):
    """int32 [B, M]: each row's first ``pages_per_row`` entries are
    distinct physical pages drawn from a seeded permutation of
    1..num_pages-1; the unused entries stay 0."""
    g = torch.Generator().manual_seed(seed)
    perm = (torch.randperm(num_pages - 1, generator=g) + 1).to(torch.int32)
    assert B * pages_per_row <= num_pages - 1
    bt = torch.zeros(B, M, dtype=torch.int32)
    bt[:, :pages_per_row] = perm[:B * pages_per_row].reshape(B, pages_per_row)
    return bt.to(device)


def _gather_dense(pool, bt, T):
    """Dense [B, T, Hkv, D] view of the logical caches."""
    return torch.cat([reference.paged_gather(pool, bt[b], T)
                      for b in range(bt.shape[0])], dim=0).contiguous()


# ---------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------


def test_page_allocator():
    a = PageAllocator(6)
    assert a.num_free == 5                       # page 0 is reserved
    first = a.alloc(2)
    assert 0 not in first and len(set(first)) == 2
    with pytest.raises(OutOfPages):
        a.alloc(4)                               # only 3 left
    assert a.num_free == 3                       # all-or-nothing
    rest = a.alloc(3)
    assert sorted(first + rest) == [1, 2, 3, 4, 5]
    with pytest.raises(OutOfPages):
        a.alloc(1)
    # LIFO: the page freed last is handed out first
    a.free([first[0]])
    a.free([rest[1]])
    assert a.alloc(1) == [rest[1]]
    assert a.alloc(1) == [first[0]]
    with pytest.raises(AssertionError):
        a.free([0])
    a.free([first[1]])
    with pytest.raises(AssertionError):
        a.free([first[1]])                       # double free
    a.free([first[0]] + rest)
    assert a.num_free == 5
    for _ in range(3):
        a.free(a.alloc(5))
    assert a.num_free == 5


def test_paged_ops_cpu_equal_dense():
    torch.manual_seed(21)
    B, Hq, Hkv, D, P, M, num_pages = 3, 4, 2, 64, 16, 5, 12
    pos = torch.tensor([0, 20, 37], dtype=torch.int32)
    bt = _shuffled_table(B, 3, M, num_pages, seed=5)   # 3 pages cover pos 37
    kpool = torch.randn(num_pages, P, Hkv, D).to(torch.bfloat16)
    vpool = torch.randn(num_pages, P, Hkv, D).to(torch.bfloat16)
    q = torch.randn(B, Hq, D).to(torch.bfloat16)
    kc, vc = _gather_dense(kpool, bt, 3 * P), _gather_dense(vpool, bt, 3 * P)
    o = ops.paged_decode_attention(q, kpool, vpool, bt, pos)
    assert torch.equal(o, ops.decode_attention_dev(q, kc, vc, pos))

    # rope + append: sentinel-filled pools, only B slots may change
    cos, sin = ops.rope_tables(64, D)
    qkv = torch.randn(B, (Hq + 2 * Hkv) * D).to(torch.bfloat16)
    kp = torch.full((num_pages, P, Hkv, D), 7.0, dtype=torch.bfloat16)
    vp = torch.full_like(kp, -3.0)
    kd = torch.full((B, 3 * P, Hkv, D), 7.0, dtype=torch.bfloat16)
    vd = torch.full_like(kd, -3.0)
    qp = ops.paged_decode_rope_cache(qkv, kp, vp, bt, cos, sin, pos, Hq)
    qd = ops.decode_rope_cache(qkv, kd, vd, cos, sin, pos, Hq)
    assert torch.equal(qp, qd)
    assert torch.equal(_gather_dense(kp, bt, 3 * P), kd)
    assert torch.equal(_gather_dense(vp, bt, 3 * P), vd)
    kexp = torch.full_like(kp, 7.0)
    vexp = torch.full_like(vp, -3.0)
    for b in range(B):
        p = int(pos[b])
        kexp[int(bt[b, p // P]), p % P] = kd[b, p]
        vexp[int(bt[b, p // P]), p % P] = vd[b, p]
    assert torch.equal(kp, kexp)
    assert torch.equal(vp, vexp)


def test_paged_batcher_matches_per_sequence():
    """Pages are allocated mid-decode (13->21 crosses 16, 30->38 crosses
    32); after a retire, a new prompt in ANOTHER row reuses the freed
    pages while the retired row idles on the dump page."""
    torch.manual_seed(31)
    cfg = llama_tiny()
    model = LlamaModel(cfg)
    p1 = torch.randint(0, cfg.vocab_size, (13,))
    p2 = torch.randint(0, cfg.vocab_size, (30,))
    p3 = torch.randint(0, cfg.vocab_size, (7,))
    solo1 = generate(model, p1.reshape(1, -1), 9)[0, 13:].tolist()
    solo2 = generate(model, p2.reshape(1, -1), 15)[0, 30:].tolist()
    solo3 = generate(model, p3.reshape(1, -1), 7)[0, 7:].tolist()

    pb = PagedBatcher(model, max_batch=3, max_len=64, num_pages=10,
                      page_size=16)
    free0 = pb.free_pages()
    got1, got2 = [int(pb.admit(0, p1))], [int(pb.admit(1, p2))]
    assert free0 - pb.free_pages() == 1 + 2
    for _ in range(8):
        toks = pb.step()
        got1.append(int(toks[0]))
        got2.append(int(toks[1]))
    assert free0 - pb.free_pages() == 2 + 3      # one more page each
    assert got1 == solo1, (got1, solo1)
    assert got2 == solo2[:9], (got2, solo2)

    row0_pages = list(pb.pages[0])
    pb.retire(0)
    assert pb.free_rows() == [0, 2]
    assert pb.block_table[0].tolist() == [0] * pb.table_width
    got3 = [int(pb.admit(2, p3))]
    assert pb.pages[2] == [row0_pages[-1]]       # LIFO reuse of row 0's page
    more2 = []
    for _ in range(6):
        toks = pb.step()
        got3.append(int(toks[2]))
        more2.append(int(toks[1]))
    assert got3 == solo3, (got3, solo3)
    assert more2 == solo2[9:], (more2, solo2)
    assert int(pb.pos[0]) == 0                   # the retired row stood still


def test_paged_batcher_pressure():
    torch.manual_seed(41)
    cfg = llama_tiny()
    model = LlamaModel(cfg)
    # 5 usable pages = 80 rows; a dense pool would hold 3 * 96 = 288
    pb = PagedBatcher(model, max_batch=3, max_len=96, num_pages=6,
                      page_size=16)
    free0 = pb.free_pages()
    assert free0 == 5
    pb.admit(0, torch.randint(0, cfg.vocab_size, (30,)))   # 2 pages
    pb.admit(1, torch.randint(0, cfg.vocab_size, (20,)))   # 2 pages
    assert pb.free_pages() == 1
    table = pb.block_table.clone()
    with pytest.raises(OutOfPages):
        pb.admit(2, torch.randint(0, cfg.vocab_size, (18,)))  # needs 2
    assert pb.free_pages() == 1
    assert torch.equal(pb.block_table, table)
    assert pb.free_rows() == [2]
    # row 0 enters its third page at pos 32 (step 3) and takes the last
    # free page; row 1 needs one at pos 32 (step 13) and finds none
    for _ in range(12):
        pb.step()
    assert pb.free_pages() == 0 and pb.preempted == []
    assert len(pb.pages[0]) == 3 and len(pb.pages[1]) == 2
    pb.step()
    assert pb.preempted == [1]
    assert not pb.active[1] and pb.active[0]
    assert pb.free_pages() == 2                  # row 1's pages came back
    assert pb.block_table[1].tolist() == [0] * pb.table_width
    pb.retire(0)
    assert pb.free_pages() == free0


def test_paged_batcher_mixtral_matches_continuous():
    from torchx_amd.models.generate_moe import decode_step_moe, prefill_moe
    from torchx_amd.models.mixtral import MixtralModel, mixtral_tiny

    torch.manual_seed(51)
    cfg = mixtral_tiny()
    model = MixtralModel(cfg)
    p1 = torch.randint(0, cfg.vocab_size, (13,))
    p2 = torch.randint(0, cfg.vocab_size, (30,))
    kw = dict(prefill_fn=prefill_moe, decode_fn=decode_step_moe)
    cb = ContinuousBatcher(model, max_batch=2, max_len=64, **kw)
    pb = PagedBatcher(model, max_batch=2, max_len=64, num_pages=8,
                      page_size=16, **kw)
    want, got = [], []
    for b, out in ((cb, want), (pb, got)):
        out.append([int(b.admit(0, p1)), int(b.admit(1, p2))])
        for _ in range(6):
            out.append(b.step().tolist())
    assert got == want, (got, want)


# ---------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------

_ATTN_CASES = {
    # name: (B, Hq, Hkv, P, pos)
    "split16_p16": (3, 8, 4, 16, [0, 76, 200]),
    "split16_p64": (3, 8, 4, 64, [0, 76, 200]),
    "single_pass": (8, 64, 8, 16, [0, 5, 15, 16, 17, 31, 33, 40]),
    "long_cache": (2, 4, 2, 16, [1100, 530]),
}


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(_ATTN_CASES))
def test_paged_decode_attention_gpu_bit_identical(case):
    B, Hq, Hkv, P, pos_l = _ATTN_CASES[case]
    D = 128
    dev = torch.device("cuda:0")
    torch.manual_seed(61)
    n = max(pos_l) // P + 1                       # pages per row
    M = n + 2                                     # unused entries stay 0
    num_pages = B * n + 3
    bt = _shuffled_table(B, n, M, num_pages, seed=6, device=dev)
    pos = torch.tensor(pos_l, dtype=torch.int32, device=dev)
    kpool = torch.randn(num_pages, P, Hkv, D, device=dev,
                        dtype=torch.bfloat16)
    vpool = torch.randn(num_pages, P, Hkv, D, device=dev,
                        dtype=torch.bfloat16)
    q = torch.randn(B, Hq, D, device=dev, dtype=torch.bfloat16)
    kc, vc = _gather_dense(kpool, bt, n * P), _gather_dense(vpool, bt, n * P)
    o = ops.paged_decode_attention(q, kpool, vpool, bt, pos)
    dense = ops.decode_attention_dev(q, kc, vc, pos)
    qc, kcc, vcc = q.cpu(), kc.cpu(), vc.cpu()
    ref = torch.cat([reference.decode_attention(
        qc[b:b + 1], kcc[b:b + 1], vcc[b:b + 1], pos_l[b] + 1, 1.0 / D ** 0.5)
        for b in range(B)], dim=0)
    err = (o.cpu().float() - ref.float()).abs().max().item()
    print(f"{case}: max abs err vs fp32 reference {err:.3e}, "
          f"bit-identical to dense: {torch.equal(o, dense)}")
    assert torch.equal(o, dense)
    assert err < 3e-2, err


@pytest.mark.gpu
def test_paged_decode_rope_cache_gpu_bit_identical():
    dev = torch.device("cuda:0")
    torch.manual_seed(71)
    B, Hq, Hkv, D, P, M, num_pages = 3, 8, 4, 128, 16, 4, 9
    pos_l = [0, 17, 31]
    pos = torch.tensor(pos_l, dtype=torch.int32, device=dev)
    bt = _shuffled_table(B, 2, M, num_pages, seed=7, device=dev)
    qkv = torch.randn(B, (Hq + 2 * Hkv) * D, device=dev,
                      dtype=torch.bfloat16)
    cos, sin = ops.rope_tables(64, D, device=dev)
    kp = torch.full((num_pages, P, Hkv, D), 7.0, device=dev,
                    dtype=torch.bfloat16)
    vp = torch.full_like(kp, -3.0)
    kd = torch.full((B, 2 * P, Hkv, D), 7.0, device=dev,
                    dtype=torch.bfloat16)
    vd = torch.full_like(kd, -3.0)
    qp = ops.paged_decode_rope_cache(qkv, kp, vp, bt, cos, sin, pos, Hq)
    qd = ops.decode_rope_cache(qkv, kd, vd, cos, sin, pos, Hq)
    assert torch.equal(qp, qd)
    assert torch.equal(_gather_dense(kp, bt, 2 * P), kd)
    assert torch.equal(_gather_dense(vp, bt, 2 * P), vd)
    kexp = torch.full_like(kp, 7.0)
    vexp = torch.full_like(vp, -3.0)
    btc = bt.cpu()
    for b, p in enumerate(pos_l):
        kexp[int(btc[b, p // P]), p % P] = kd[b, p]
        vexp[int(btc[b, p // P]), p % P] = vd[b, p]
    assert torch.equal(kp, kexp)
    assert torch.equal(vp, vexp)


@pytest.mark.gpu
def test_paged_batcher_gpu_matches_per_sequence():
    from torchx_amd.models.llama import llama_gpu_tiny

    dev = torch.device("cuda:0")
    torch.manual_seed(81)
    cfg = llama_gpu_tiny()
    model = LlamaModel(cfg, device=dev)
    p1 = torch.randint(0, cfg.vocab_size, (24,), device=dev)
    p2 = torch.randint(0, cfg.vocab_size, (40,), device=dev)
    p3 = torch.randint(0, cfg.vocab_size, (9,), device=dev)
    solo1 = generate(model, p1.reshape(1, -1), 11)[0, 24:].tolist()
    solo2 = generate(model, p2.reshape(1, -1), 16)[0, 40:].tolist()
    solo3 = generate(model, p3.reshape(1, -1), 6)[0, 9:].tolist()

    pb = PagedBatcher(model, max_batch=2, max_len=96, num_pages=12,
                      page_size=16)
    free0 = pb.free_pages()
    got1, got2 = [int(pb.admit(0, p1))], [int(pb.admit(1, p2))]
    for _ in range(10):                           # crosses 32 and 48
        toks = pb.step().tolist()
        got1.append(toks[0])
        got2.append(toks[1])
    assert free0 - pb.free_pages() == 3 + 4
    assert got1 == solo1, (got1, solo1)
    assert got2 == solo2[:11], (got2, solo2)
    freed = list(pb.pages[0])
    pb.retire(0)
    got3 = [int(pb.admit(0, p3))]
    assert pb.pages[0] == [freed[-1]]             # reuses a freed page
    more2 = []
    for _ in range(5):
        toks = pb.step().tolist()
        got3.append(toks[0])
        more2.append(toks[1])
    assert got3 == solo3, (got3, solo3)
    assert more2 == solo2[11:], (more2, solo2)
