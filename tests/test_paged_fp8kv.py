"""Paged fp8 KV cache (ops/csrc/paged_attn_fp8kv.hip): the block-table
attention kernel bit for bit against the dense fp8 kernel and under its
fp64 bound over pools poisoned wherever no valid row lies, the two paged
quantisers bit for bit against ``ops.quantize_kv_rows``, and
``PagedBatcher(kv_cache="fp8")`` token for token against
``ContinuousBatcher(kv_cache="fp8")``."""

import pytest
import torch

from torchx_amd import ops
from torchx_amd.ops import bounds as bd

DEV = "cuda:0"
T = 320  # logical cache rows

# (id, Hq, Hkv, P, lengths, split, rows_hint); split None = the policy
ATTN_CASES = [
    ("g1-L1", 4, 4, 16, (1, 1), 1, None),
    ("g4-L33", 8, 2, 16, (33, 33), 1, None),
    ("g8-P64-L129", 8, 1, 64, (129,), 1, None),
    ("g4-L300", 8, 2, 16, (300, 300), 1, None),
    ("g4-ragged-split5", 8, 2, 16, (1, 77, 300), 5, None),
    ("g2-P256-split2", 4, 2, 256, (300, 300), 2, None),
    ("g4-P32-policy", 8, 2, 32, (300, 300), None, 300),
]


def _shuffled_table(B, M, seed, device):
    """int32 [B, M] over the pages 1 .. B*M in a seeded order."""
    g = torch.Generator().manual_seed(seed)
    return (torch.randperm(B * M, generator=g) + 1).reshape(B, M).to(
        torch.int32).to(device)


def _scatter(pool, dense, table, lengths, start=0):
    """Logical rows start .. start+lengths[b]-1 of sequence b take
    dense[b, :lengths[b]] [n, ...], through ``table``, into ``pool``
    [num_pages, P, ...]."""
    P = pool.shape[1]
    for b, n in enumerate(lengths):
        t = torch.arange(start, start + n, device=pool.device)
        pool[table[b, t // P].long(), t % P] = dense[b, :n]


def _bytes(x8):
    return x8.view(torch.uint8)


@pytest.mark.gpu
@pytest.mark.parametrize("family", bd.FAMILIES)
@pytest.mark.parametrize("case", ATTN_CASES, ids=[c[0] for c in ATTN_CASES])
def test_paged_attention_equals_dense_within_bound(case, family):
    """Every pool row that holds no valid cache row (page 0, unowned pages,
    owned rows at or past the length) is e4m3 NaN bytes under a NaN scale
    and unused table entries are 0, so one read outside the valid rows
    fails both checks."""
    cid, Hq, Hkv, P, lengths, split, rows_hint = case
    B, M = len(lengths), -(-T // P)
    q, kc, vc = bd.decode_inputs(family, B, Hq, Hkv, T,
                                 seed=bd.case_seed(cid), device=DEV)
    (k8, ks), (v8, vs) = ops.quantize_kv_rows(kc), ops.quantize_kv_rows(vc)
    ref = bd.decode_fp8kv_ref_bound(q, k8, v8, ks, vs, lengths, bd.SCALE)

    table = _shuffled_table(B, M, 1, DEV)
    for b, n in enumerate(lengths):
        table[b, -(-n // P):] = 0
    pools8 = [torch.full((B * M + 1, P, Hkv, 128), 0x7f, dtype=torch.uint8,
                         device=DEV) for _ in range(2)]
    pools = [torch.full((B * M + 1, P, Hkv), float("nan"), device=DEV)
             for _ in range(2)]
    for pool, dense in zip(pools8 + pools, (_bytes(k8), _bytes(v8), ks, vs)):
        _scatter(pool, dense, table, lengths)
    pos = torch.tensor(lengths, dtype=torch.int32, device=DEV) - 1
    o = ops.paged_decode_attention_fp8kv(
        q, *(p.view(torch.float8_e4m3fn) for p in pools8), *pools, table,
        pos, bd.SCALE, split=split, rows_hint=rows_hint)
    assert o.shape == q.shape and o.dtype == torch.bfloat16
    if split is not None:
        twin = ops.decode_attention_fp8kv(
            q, k8, v8, ks, vs, lengths[0] if len(set(lengths)) == 1 else pos,
            bd.SCALE, split=split)
        assert torch.equal(o, twin), cid
    ratio, ok = bd.bound_ratio(o, ref["o"], ref["o_bound"])
    print(f"paged_decode_attention_fp8kv {cid} {family}: "
          f"max err/bound {ratio:.3f}")
    assert ok, (cid, family, ratio)


def _spread_rows(shape, seed, zero=(0, 0), outlier=(0, 1)):
    """test_decode_fp8kv's quantiser inputs: randn [B, N, D] rows with
    magnitudes spread over 2^+-6, the rows ``zero`` ((b, n) pairs) all zero
    and the rows ``outlier`` with one element 1000 times the rest."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(shape, generator=g)
    x *= 2.0 ** (torch.rand(shape[:-1], generator=g) * 12 - 6)[..., None]
    for b, n in zip(zero[::2], zero[1::2]):
        x[b, n] = 0.0
    for b, n in zip(outlier[::2], outlier[1::2]):
        x[b, n, 5] = 1000.0 * x[b, n].abs().max()
    return x.to(torch.bfloat16).to(DEV)


@pytest.mark.gpu
@pytest.mark.parametrize("S,start", [(5, 0), (40, 7)])
@pytest.mark.parametrize("P", [16, 64])
def test_paged_quantisers_bit_exact(P, S, start):
    """The store and the append put ``quantize_kv_rows`` of the rows the
    bf16 ops produce, bytes and scales, where the table says; every other
    pool row keeps its sentinel and q is the bf16 op's q."""
    B, Hq, Hkv, D, Tc = 3, 8, 2, 128, 80
    M = -(-Tc // P)
    cos, sin = ops.rope_tables(Tc, D, device=DEV)
    k = ops.rope(_spread_rows((B, S * Hkv, D), 1).view(B, S, Hkv, D),
                 cos[start:start + S], sin[start:start + S])
    v = _spread_rows((B, S * Hkv, D), 2).view(B, S, Hkv, D)
    # heads of a qkv row: q 0..7, k 8..9, v 10..11
    qkv = _spread_rows((B, Hq + 2 * Hkv, D), 3, zero=(0, Hq, 1, Hq + 3),
                       outlier=(1, Hq + 1, 2, Hq + 2)).reshape(B, -1)
    pos = [start + S + b for b in range(B)]
    pos_dev = torch.tensor(pos, dtype=torch.int32, device=DEV)
    table = _shuffled_table(B, M, 2, DEV)

    k8p = torch.full((B * M + 1, P, Hkv, D), 0.75,
                     device=DEV).to(torch.float8_e4m3fn)
    ksp = torch.full((B * M + 1, P, Hkv), 3.0, device=DEV)
    got = [k8p, k8p.clone(), ksp, ksp.clone()]
    want = [_bytes(got[0]).clone(), _bytes(got[1]).clone(), ksp.clone(),
            ksp.clone()]
    ops.paged_kv_quantize_store(k, v, *got, table, start)
    kc = torch.zeros(B, Tc, Hkv, D, dtype=torch.bfloat16, device=DEV)
    vc = torch.zeros_like(kc)
    q16 = ops.decode_rope_cache(qkv, kc, vc, cos, sin, pos_dev, Hq)
    q8 = ops.paged_decode_rope_cache_fp8kv(qkv, *got, table, cos, sin,
                                           pos_dev, Hq)
    assert torch.equal(q8, q16)
    for i, (stored, appended) in enumerate(((k, kc), (v, vc))):
        x8, xs = ops.quantize_kv_rows(stored)
        _scatter(want[i], _bytes(x8), table, [S] * B, start)
        _scatter(want[2 + i], xs, table, [S] * B, start)
        for b, p in enumerate(pos):
            a8, a_s = ops.quantize_kv_rows(appended[b:b + 1, p:p + 1])
            _scatter(want[i], _bytes(a8), table[b:b + 1], [1], p)
            _scatter(want[2 + i], a_s, table[b:b + 1], [1], p)
    for name, g, w in zip(("k8", "v8", "ks", "vs"), got, want):
        g = g if g.dtype == torch.float32 else _bytes(g)
        assert torch.equal(g, w), name


def _serve(batcher, prompts):
    """Rows admitted at different steps, then a retire and a re-admit into
    the freed pages; the tokens of the live rows, in order."""
    out = [int(batcher.admit(0, prompts[0]))]
    out += [int(batcher.step()[0]) for _ in range(3)]
    out.append(int(batcher.admit(1, prompts[1])))
    out += [t for _ in range(5) for t in batcher.step()[:2].tolist()]
    batcher.retire(0)
    out += [int(batcher.step()[1]) for _ in range(2)]
    out.append(int(batcher.admit(0, prompts[1])))
    out += [t for _ in range(4) for t in batcher.step()[:2].tolist()]
    return out


def _batchers_agree(cfg, device):
    from torchx_amd.models.generate import ContinuousBatcher, PagedBatcher
    from torchx_amd.models.llama import LlamaModel

    torch.manual_seed(21)
    model = LlamaModel(cfg, device=device)
    prompts = [torch.randint(0, cfg.vocab_size, (n,), device=device)
               for n in (24, 37)]
    dense = _serve(ContinuousBatcher(model, 2, 96, kv_cache="fp8"), prompts)
    pb = PagedBatcher(model, 2, 96, num_pages=7, page_size=16, kv_cache="fp8")
    assert _serve(pb, prompts) == dense
    # 2 + 3 pages, then 3 + 3 of the 6: the re-admit needs the freed ones
    assert pb.free_pages() == 0 and not pb.preempted


@pytest.mark.gpu
def test_paged_batcher_fp8_matches_dense_batcher():
    """Exact: both split policies give 1 below 128 rows, the prefill is the
    same kernel, and the stored bytes and the decode kernels are
    bit-identical."""
    from torchx_amd.models.llama import llama_gpu_tiny

    _batchers_agree(llama_gpu_tiny(), DEV)


def test_paged_batcher_fp8_matches_dense_batcher_cpu():
    from torchx_amd.models.llama import llama_tiny

    _batchers_agree(llama_tiny(), "cpu")


def test_cpu_fallbacks_equal_dense_ops_on_gathered_cache():
    B, Hq, Hkv, D, P, M, S = 2, 4, 2, 128, 16, 3, 21
    g = torch.Generator().manual_seed(5)
    k, v = (torch.randn(B, S, Hkv, D, generator=g).bfloat16()
            for _ in range(2))
    qkv = torch.randn(B, (Hq + 2 * Hkv) * D, generator=g).bfloat16()
    cos, sin = ops.rope_tables(M * P, D)
    table = _shuffled_table(B, M, 3, "cpu")
    pos = torch.tensor([S, S + 1], dtype=torch.int32)
    pools = [torch.zeros(B * M + 1, P, Hkv, D).to(torch.float8_e4m3fn)
             for _ in range(2)] + [torch.zeros(B * M + 1, P, Hkv)
                                   for _ in range(2)]
    dense = [torch.zeros(B, M * P, Hkv, D).to(torch.float8_e4m3fn)
             for _ in range(2)] + [torch.zeros(B, M * P, Hkv)
                                   for _ in range(2)]
    ops.paged_kv_quantize_store(k, v, *pools, table, 2)
    ops.kv_quantize_store(k, v, *dense, 2)
    qp = ops.paged_decode_rope_cache_fp8kv(qkv, *pools, table, cos, sin, pos,
                                           Hq)
    qd = ops.decode_rope_cache_fp8kv(qkv, *dense, cos, sin, pos, Hq)
    assert torch.equal(qp, qd)
    for b in range(B):
        for p, d in zip(ops._paged_gather_fp8kv(*pools, table[b], M * P),
                        dense):
            same = torch.equal(p[0].float(), d[b].float())
            assert same, b
    assert torch.equal(
        ops.paged_decode_attention_fp8kv(qp, *pools, table, pos),
        ops.decode_attention_fp8kv(qd, *dense, pos))


@pytest.mark.parametrize("option", ["prefix_sharing", "prefill_chunk",
                                    "admit_many"])
def test_fp8_pools_refuse_the_bf16_prefill_paths(option):
    from torchx_amd.models.generate import PagedBatcher
    from torchx_amd.models.llama import LlamaModel, llama_tiny

    model = LlamaModel(llama_tiny())
    kw = {"prefix_sharing": {"prefix_sharing": True},
          "prefill_chunk": {"prefill_chunk": 8}, "admit_many": {}}[option]
    with pytest.raises(AssertionError, match="fp8 prefill kernels"):
        pb = PagedBatcher(model, 2, 64, 9, kv_cache="fp8", **kw)
        pb.admit_many([0], [torch.arange(5)])
