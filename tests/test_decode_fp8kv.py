"""fp8 KV cache for dense decode (ops/csrc/decode_attn_fp8kv.hip): the
attention kernel against the fp64 reference on the dequantised cache under
``bounds.decode_fp8kv_ref_bound``, the two quantisers bit for bit against
``ops.quantize_kv_rows``, and the serving path end to end."""

import pytest
import torch

from torchx_amd import ops
from torchx_amd.ops import bounds as bd

DEV = "cuda:0"
T = 320  # cache rows: the launcher's own split is min(.., T // 128) = 2

# (id, B, Hq, Hkv, lengths, split); split None = the launcher's policy,
# 2 here, so those cases run slices of ceil(L / 2) rows. L = 1: one row,
# every other slot empty; 31 / 33 under the policy: 16- and 17-row slices,
# empty slots in the only iteration; 129 single-pass: one unmasked 128-row
# group plus a one-row tail (the main loop of the G = 1, 2 and 8 instances;
# G = 4 has it at L = 300); 40 single-pass: either side of one 32-row
# iteration in one slice; 300 under the policy: two 150-row slices, each a
# group and a tail that ends mid-iteration; split 8 / 5: 38- and 60-row
# slices (tail only).
ATTN_CASES = [
    ("g1-L1", 2, 4, 4, (1, 1), None),
    ("g4-L31", 2, 8, 2, (31, 31), None),
    ("g4-L33", 2, 8, 2, (33, 33), None),
    ("g4-L40-single", 2, 8, 2, (40, 40), 1),
    ("g1-L129-single", 2, 4, 4, (129, 129), 1),
    ("g2-L129-single", 2, 4, 2, (129, 129), 1),
    ("g8-L129-single", 1, 8, 1, (129,), 1),
    ("g8-L300", 2, 16, 2, (300, 300), None),
    ("g4-ragged", 3, 8, 2, (1, 77, 300), None),
    ("g1-L300-split8", 2, 4, 4, (300, 300), 8),
    ("g4-L300-split5", 2, 8, 2, (300, 300), 5),
    ("g4-L300-single", 2, 8, 2, (300, 300), 1),
]


def _fp8_cache(family, cid, B, Hq, Hkv):
    q, kc, vc = bd.decode_inputs(family, B, Hq, Hkv, T,
                                 seed=bd.case_seed(cid), device=DEV)
    return (q,) + ops.quantize_kv_rows(kc) + ops.quantize_kv_rows(vc)


def _within(name, got, ref):
    ratio, ok = bd.bound_ratio(got, ref["o"], ref["o_bound"])
    print(f"{name}: max err/bound {ratio:.3f}")
    assert ok, (name, ratio)


@pytest.mark.gpu
@pytest.mark.parametrize("family", bd.FAMILIES)
@pytest.mark.parametrize("case", ATTN_CASES, ids=[c[0] for c in ATTN_CASES])
def test_attention_within_bound(case, family):
    """``stepped``: k[t, 0] climbs by 7 every 16 rows, so the maximum of
    every 128-row group, of every tail iteration behind one and of every
    later slice exceeds the running one: the once-per-group alpha rescales
    a live accumulator in every group but a slot's first, and the slot,
    wave and slice merges all run with weights far from 1 (the per-group
    analogue of ``bd.rescale_coverage``, which replays the training
    kernels' per-tile decision)."""
    cid, B, Hq, Hkv, lengths, split = case
    q, k8, ks, v8, vs = _fp8_cache(family, cid, B, Hq, Hkv)
    ref = bd.decode_fp8kv_ref_bound(q, k8, v8, ks, vs, lengths, bd.SCALE)
    if len(set(lengths)) == 1:
        arg = lengths[0]
    else:
        arg = torch.tensor(lengths, dtype=torch.int32, device=DEV) - 1
    o = ops.decode_attention_fp8kv(q, k8, v8, ks, vs, arg, bd.SCALE,
                                   split=split)
    assert o.shape == q.shape and o.dtype == torch.bfloat16
    _within(f"decode_attention_fp8kv {cid} {family}", o, ref)


@pytest.mark.gpu
@pytest.mark.parametrize("family", bd.FAMILIES)
def test_split_single_and_length_forms(family):
    B, Hq, Hkv, L = 2, 8, 2, 300
    q, k8, ks, v8, vs = _fp8_cache(family, "forms", B, Hq, Hkv)
    ref = bd.decode_fp8kv_ref_bound(q, k8, v8, ks, vs, [L] * B, bd.SCALE)

    def run(arg, split=None):
        return ops.decode_attention_fp8kv(q, k8, v8, ks, vs, arg, bd.SCALE,
                                          split=split)

    _within(f"split4 {family}", run(L, 4), ref)
    _within(f"single {family}", run(L, 1), ref)
    host = run(L)
    scalar = run(torch.tensor([L - 1], dtype=torch.int32, device=DEV))
    rows = run(torch.full((B,), L - 1, dtype=torch.int32, device=DEV))
    assert torch.equal(host, scalar) and torch.equal(host, rows)


def _spread_rows(shape, seed, device=DEV, zero=(0, 0), outlier=(0, 1)):
    """randn [B, N, D] rows with magnitudes spread over 2^+-6; the rows
    ``zero`` (pairs of (b, n) indices) are all zero and the rows
    ``outlier`` have one element 1000 times the rest."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(shape, generator=g)
    x *= 2.0 ** (torch.rand(shape[:-1], generator=g) * 12 - 6)[..., None]
    for b, n in zip(zero[::2], zero[1::2]):
        x[b, n] = 0.0
    for b, n in zip(outlier[::2], outlier[1::2]):
        x[b, n, 5] = 1000.0 * x[b, n].abs().max()
    return x.to(torch.bfloat16).to(device)


def _bytes(x8):
    return x8.view(torch.uint8)


@pytest.mark.gpu
@pytest.mark.parametrize("S,start", [(5, 0), (5, 7), (64, 0), (64, 7)])
def test_quantisers_bit_exact(S, start):
    """Both quantisers equal ``quantize_kv_rows`` of the rows the bf16 ops
    produce, bytes and scales; the other cache rows keep their content and
    q is the bf16 op's q. The append runs at [B] positions behind the
    stored rows for S = 5, at a host position for S = 64."""
    B, Hq, Hkv, D, Tc = 3, 8, 2, 128, 80
    cos, sin = ops.rope_tables(Tc, D, device=DEV)
    k = ops.rope(_spread_rows((B, S * Hkv, D), 1).view(B, S, Hkv, D),
                 cos[start:start + S], sin[start:start + S])
    v = _spread_rows((B, S * Hkv, D), 2).view(B, S, Hkv, D)
    # heads of a qkv row: q 0..7, k 8..9, v 10..11. Zero rows: k head 0 of
    # b = 0, v head 1 of b = 1; outlier rows: k head 1 of b = 1, v head 0
    # of b = 2
    qkv = _spread_rows((B, Hq + 2 * Hkv, D), 3, zero=(0, Hq, 1, Hq + 3),
                       outlier=(1, Hq + 1, 2, Hq + 2)).reshape(B, -1)
    pos = [start + S + b for b in range(B)] if S == 5 else [start + S] * B
    pos_arg = (torch.tensor(pos, dtype=torch.int32, device=DEV) if S == 5
               else pos[0])

    k8 = torch.full((B, Tc, Hkv, D), 0.75, device=DEV).to(torch.float8_e4m3fn)
    v8 = k8.clone()
    ks = torch.full((B, Tc, Hkv), 3.0, device=DEV)
    vs = ks.clone()
    want = [t.clone() for t in (k8, ks, v8, vs)]
    ops.kv_quantize_store(k, v, k8, v8, ks, vs, start)
    want[0][:, start:start + S], want[1][:, start:start + S] = \
        ops.quantize_kv_rows(k)
    want[2][:, start:start + S], want[3][:, start:start + S] = \
        ops.quantize_kv_rows(v)

    kc = torch.zeros(B, Tc, Hkv, D, dtype=torch.bfloat16, device=DEV)
    vc = torch.zeros_like(kc)
    q16 = ops.decode_rope_cache(qkv, kc, vc, cos, sin, pos_arg, Hq)
    q8 = ops.decode_rope_cache_fp8kv(qkv, k8, v8, ks, vs, cos, sin, pos_arg,
                                     Hq)
    for b, p in enumerate(pos):
        want[0][b, p], want[1][b, p] = ops.quantize_kv_rows(kc[b, p])
        want[2][b, p], want[3][b, p] = ops.quantize_kv_rows(vc[b, p])
    assert torch.equal(q8, q16)
    for name, got, exp in zip(("k8", "ks", "v8", "vs"), (k8, ks, v8, vs),
                              want):
        if got.dtype != torch.float32:
            got, exp = _bytes(got), _bytes(exp)
        assert torch.equal(got, exp), name


@pytest.mark.gpu
def test_decode_step_fp8kv_end_to_end(monkeypatch):
    """One decode step after a 16-token prefill, over an fp8 and over a bf16
    cache, each against the same step on the CPU in fp32 over a copy of its
    own cache (the fp8 one through the CPU path, which attends the fp32
    dequantised rows): max|fp8kv - ref| <= 2 max|bf16 - ref|, the margin of
    test_decode_step_fp8_weights_end_to_end for the summation orders. Same
    2-layer config, B = 3. The row the step itself appends is cached too,
    so the fp8 reference attends a copy of the cache taken AFTER the GPU
    step and its own append goes to clones: a value that the GPU (from
    bf16) and the CPU (from fp32) quantise to neighbouring e4m3 codes, a 6%
    step, would bring the quantisation error back in. decode_step has no
    form that attends without appending, hence the patch; the appended row
    is held to ``quantize_kv_rows`` bit for bit above."""
    from torchx_amd.models.generate import (
        Fp8KVCache, KVCache, decode_step, prefill,
    )
    from torchx_amd.models.llama import LlamaConfig, LlamaModel

    torch.manual_seed(11)
    cfg = LlamaConfig(vocab_size=512, hidden_size=2048, intermediate_size=2048,
                      num_layers=2, num_heads=8, num_kv_heads=2, head_dim=128,
                      max_seq_len=64)
    B, S, Tc = 3, 16, 32
    model = LlamaModel(cfg, device=DEV)
    ref_model = LlamaModel(cfg)
    ref_model.load_state_dict(model.state_dict())
    ref_model.float()
    tokens = torch.randint(0, cfg.vocab_size, (B, S), device=DEV)
    errs = {}
    for kind in (Fp8KVCache, KVCache):
        caches = [kind.empty(cfg, B, Tc, DEV) for _ in range(cfg.num_layers)]
        nxt = prefill(model, tokens, caches).argmax(-1, keepdim=True)
        if kind is KVCache:
            ref_caches = [KVCache(c.k.cpu().float(), c.v.cpu().float(), S)
                          for c in caches]
        got = decode_step(model, nxt, caches).double().cpu()
        if kind is Fp8KVCache:
            ref_caches = [Fp8KVCache(c.k8.cpu(), c.v8.cpu(), c.ks.cpu(),
                                     c.vs.cpu(), S) for c in caches]
            monkeypatch.setattr(
                ops, "decode_rope_cache_fp8kv",
                lambda qkv, k8, v8, ks, vs, *a, fn=ops.decode_rope_cache_fp8kv:
                fn(qkv, k8.clone(), v8.clone(), ks.clone(), vs.clone(), *a))
        ref = decode_step(ref_model, nxt.cpu(), ref_caches).double()
        monkeypatch.undo()
        errs[kind] = (got - ref).abs().max().item()
    d8, d16 = errs[Fp8KVCache], errs[KVCache]
    print(f"decode step max|logits - ref|: fp8 kv {d8:.4g}, bf16 kv {d16:.4g}")
    assert d8 <= 2 * d16, (d8, d16)


@pytest.mark.gpu
def test_generate_fp8kv_matches_batcher_and_graph():
    from torchx_amd.models.generate import (
        ContinuousBatcher, generate, generate_graphed,
    )
    from torchx_amd.models.llama import LlamaModel, llama_gpu_tiny

    torch.manual_seed(12)
    cfg = llama_gpu_tiny()
    model = LlamaModel(cfg, device=DEV)
    p = torch.randint(0, cfg.vocab_size, (24,), device=DEV)
    solo = generate(model, p.reshape(1, -1), 8, kv_cache="fp8")[0, 24:]
    cb = ContinuousBatcher(model, max_batch=2, max_len=32, kv_cache="fp8")
    got = [int(cb.admit(0, p))] + [int(cb.step()[0]) for _ in range(7)]
    assert got == solo.tolist(), (got, solo.tolist())
    graphed = generate_graphed(model, p.reshape(1, -1), 8, kv_cache="fp8")
    assert graphed[0, 24:].tolist() == solo.tolist()


def test_quantize_kv_rows_properties():
    """scale = amax / 448 exactly, no NaN byte, the zero row -> zeros with
    scale 1, and |x - x8 scale| <= scale 2^-4 max(|x8|, 2^-6): e4m3 has 3
    mantissa bits, so a value in [2^e, 2^(e+1)) rounds within half the
    spacing 2^(e-3), i.e. 2^-4 2^e <= 2^-4 |x8| (a value rounded up to
    2^(e+1) moved by no more than that); below the least normal 2^-6 the
    spacing stays 2^-9, half of it 2^-4 2^-6. The fp32 quotient in front
    of the cast adds nothing for bf16 inputs: x / scale = 448 x / amax with
    8-bit significands misses a 5-bit tie point by 2^-21 relative or not
    at all, which an fp32 rounding cannot bridge."""
    x = _spread_rows((4, 6, 128), 0, "cpu")
    assert not x[0, 0].any() and x[0, 1].abs().max() == x[0, 1, 5].abs()
    x8, scale = ops.quantize_kv_rows(x)
    xf = x.double()
    amax = x.float().abs().amax(-1)
    assert x8.dtype == torch.float8_e4m3fn and scale.dtype == torch.float32
    assert torch.equal(scale[amax > 0], (amax / 448.0)[amax > 0])
    assert scale[0, 0] == 1.0 and not _bytes(x8[0, 0]).any()
    assert not ((_bytes(x8) & 0x7f) == 0x7f).any()
    sd = scale.double()[..., None]
    err = (xf - x8.double() * sd).abs()
    assert (err <= sd * 2.0 ** -4 * x8.double().abs().clamp(min=2.0 ** -6)).all()


def test_generate_fp8kv_cpu():
    from torchx_amd.models.generate import ContinuousBatcher, generate
    from torchx_amd.models.llama import LlamaModel, llama_tiny

    torch.manual_seed(3)
    cfg = llama_tiny()
    model = LlamaModel(cfg)
    p = torch.randint(0, cfg.vocab_size, (11,))
    out = generate(model, p.reshape(1, -1), 5, kv_cache="fp8")
    assert out.shape == (1, 16) and torch.equal(out[0, :11], p)
    cb = ContinuousBatcher(model, max_batch=2, max_len=32, kv_cache="fp8")
    got = [int(cb.admit(1, p))] + [int(cb.step()[1]) for _ in range(4)]
    assert got == out[0, 11:].tolist()
