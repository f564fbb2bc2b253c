"""KV-cache generation (serving path): the cached decode must agree with
a full re-forward at every step, on the CPU reference kernels here and on
the HIP kernels in the gpu test."""

import pytest
import torch

from torchx_amd.models.generate import KVCache, decode_step, generate, prefill
from torchx_amd.models.llama import LlamaModel, llama_tiny


def _logits_match(model, tokens, caches, new_tok):
    """decode_step logits vs full-forward logits at the same position."""
    dec = decode_step(model, new_tok, caches)
    full_in = torch.cat([tokens, new_tok], dim=1)
    with torch.no_grad():
        full = model(full_in)[:, -1]
    return dec, full, full_in


def test_cached_decode_matches_full_forward():
    torch.manual_seed(0)
    cfg = llama_tiny()
    model = LlamaModel(cfg)
    B, S0 = 2, 16
    tokens = torch.randint(0, cfg.vocab_size, (B, S0))
    caches = [KVCache.empty(cfg, B, S0 + 8, torch.device("cpu"))
              for _ in range(cfg.num_layers)]
    pre = prefill(model, tokens, caches)
    with torch.no_grad():
        full = model(tokens)[:, -1]
    assert torch.allclose(pre.float(), full.float(), atol=2e-2), (
        (pre - full).abs().max())

    cur = tokens
    nxt = pre.argmax(-1, keepdim=True)
    for _ in range(3):
        dec, full, cur = _logits_match(model, cur, caches, nxt)
        assert torch.allclose(dec.float(), full.float(), atol=3e-2), (
            (dec - full).abs().max())
        nxt = dec.argmax(-1, keepdim=True)


def test_generate_shapes_and_determinism():
    torch.manual_seed(1)
    cfg = llama_tiny()
    model = LlamaModel(cfg)
    tokens = torch.randint(0, cfg.vocab_size, (2, 8))
    out = generate(model, tokens, max_new_tokens=5)
    assert out.shape == (2, 13)
    assert torch.equal(out[:, :8], tokens)
    # greedy is deterministic
    out2 = generate(model, tokens, max_new_tokens=5)
    assert torch.equal(out, out2)
    # sampled path runs
    out3 = generate(model, tokens, max_new_tokens=3, temperature=0.8,
                    top_k=20)
    assert out3.shape == (2, 11)


@pytest.mark.gpu
def test_decode_attention_gpu_matches_reference():
    from torchx_amd import ops
    from torchx_amd.ops import reference

    dev = torch.device("cuda:0")
    torch.manual_seed(2)
    B, Hq, Hkv, T, L, D = 3, 8, 4, 96, 77, 128
    q = torch.randn(B, Hq, D, device=dev, dtype=torch.bfloat16)
    kc = torch.randn(B, T, Hkv, D, device=dev, dtype=torch.bfloat16)
    vc = torch.randn(B, T, Hkv, D, device=dev, dtype=torch.bfloat16)
    o = ops.decode_attention(q, kc, vc, L)
    ref = reference.decode_attention(q.cpu(), kc.cpu(), vc.cpu(), L,
                                     1.0 / D ** 0.5)
    err = (o.cpu().float() - ref.float()).abs().max().item()
    assert err < 3e-2, err


@pytest.mark.gpu
def test_generate_gpu_end_to_end():
    from torchx_amd.models.llama import llama_gpu_tiny

    dev = torch.device("cuda:0")
    torch.manual_seed(3)
    cfg = llama_gpu_tiny()
    model = LlamaModel(cfg, device=dev)
    tokens = torch.randint(0, cfg.vocab_size, (2, 32), device=dev)
    out = generate(model, tokens, max_new_tokens=8)
    assert out.shape == (2, 40)
    # cached decode logits agree with a full re-forward on the HIP path
    caches = [KVCache.empty(cfg, 2, 48, dev) for _ in range(cfg.num_layers)]
    prefill(model, tokens, caches)
    nxt = tokens[:, -1:]
    dec = decode_step(model, nxt, caches)
    with torch.no_grad():
        full = model(torch.cat([tokens, nxt], 1))[:, -1]
    err = (dec.float() - full.float()).abs().max().item()
    scale = full.float().abs().max().item() + 1e-6
    assert err < 5e-2 * scale, (err, scale)


@pytest.mark.gpu
def test_generate_graphed_matches_eager():
    from torchx_amd.models.generate import generate_graphed
    from torchx_amd.models.llama import llama_gpu_tiny

    dev = torch.device("cuda:0")
    torch.manual_seed(4)
    cfg = llama_gpu_tiny()
    model = LlamaModel(cfg, device=dev)
    tokens = torch.randint(0, cfg.vocab_size, (2, 24), device=dev)
    eager = generate(model, tokens, max_new_tokens=10)
    graphed = generate_graphed(model, tokens, max_new_tokens=10)
    assert eager.shape == graphed.shape, (eager.shape, graphed.shape)
    # diagnostic on divergence: also compare the FIRST decode logits of
    # both paths directly
    if not torch.equal(eager, graphed):
        from torchx_amd.models.generate import (
            GraphedDecoder, KVCache, decode_step, prefill,
        )

        div = (eager != graphed).nonzero()[:4].tolist()
        c1 = [KVCache.empty(cfg, 2, 40, dev) for _ in range(cfg.num_layers)]
        n1 = prefill(model, tokens, c1).argmax(-1, keepdim=True)
        e_log = decode_step(model, n1, c1)
        c2 = [KVCache.empty(cfg, 2, 40, dev) for _ in range(cfg.num_layers)]
        n2 = prefill(model, tokens, c2).argmax(-1, keepdim=True)
        dec = GraphedDecoder(model, c2, 2, n2, start_pos=24)
        # warm step's logits produced dec.init_tokens[0]
        raise AssertionError(
            f"streams diverge at {div}; eager tail {eager[:, 24:].tolist()} "
            f"graphed tail {graphed[:, 24:].tolist()}; "
            f"first eager tok {e_log.argmax(-1).tolist()} vs graphed warm "
            f"{dec.init_tokens[0].reshape(-1).tolist()}")


def test_decode_linear_cpu_fallback():
    from torchx_amd import ops

    x = torch.randn(2, 1, 512)
    w = torch.randn(64, 512)
    out = ops.decode_linear(x, w)
    assert out.shape == (2, 1, 64)
    assert torch.allclose(out, x @ w.t(), atol=1e-5)


@pytest.mark.gpu
def test_gemv_bf16_matches_matmul():
    from torchx_amd.ops import hip_ops

    dev = torch.device("cuda:0")
    torch.manual_seed(5)
    for M, N, K in [(1, 100, 512), (4, 4096, 1024), (8, 333, 1536),
                    (3, 17, 512), (4, 128256 // 16, 1024)]:
        x = torch.randn(M, K, device=dev, dtype=torch.bfloat16)
        w = torch.randn(N, K, device=dev, dtype=torch.bfloat16)
        out = hip_ops().gemv_bf16(x, w)
        ref = x.float() @ w.float().t()
        err = (out.float() - ref).abs().max().item()
        tol = 2e-2 * K ** 0.5
        assert err < tol, (M, N, K, err, tol)


@pytest.mark.gpu
def test_rmsnorm_res_gpu_matches_reference():
    from torchx_amd import ops

    dev = torch.device("cuda:0")
    torch.manual_seed(6)
    x = torch.randn(6, 2048, device=dev, dtype=torch.bfloat16)
    r = torch.randn(6, 2048, device=dev, dtype=torch.bfloat16)
    w = torch.randn(2048, device=dev, dtype=torch.bfloat16)
    s, y = ops.rmsnorm_res(x, r, w, 1e-5)
    s_ref = (x + r)
    n = s_ref.float()
    y_ref = (n * torch.rsqrt(n.pow(2).mean(-1, keepdim=True) + 1e-5)
             ) * w.float()
    assert torch.allclose(s.float(), s_ref.float(), atol=2e-2)
    assert torch.allclose(y.float(), y_ref, atol=3e-2), (
        (y.float() - y_ref).abs().max())
    # res=None degrades to plain rmsnorm, s aliases x
    s2, y2 = ops.rmsnorm_res(x, None, w, 1e-5)
    assert s2.data_ptr() == x.data_ptr()
    n2 = x.float()
    y2_ref = (n2 * torch.rsqrt(n2.pow(2).mean(-1, keepdim=True) + 1e-5)
              ) * w.float()
    assert torch.allclose(y2.float(), y2_ref, atol=3e-2)


@pytest.mark.gpu
def test_decode_rope_cache_gpu_matches_fallback():
    from torchx_amd import ops

    dev = torch.device("cuda:0")
    torch.manual_seed(7)
    B, Hq, Hkv, D, T, pos = 3, 8, 4, 128, 32, 17
    qkv = torch.randn(B, (Hq + 2 * Hkv) * D, device=dev,
                      dtype=torch.bfloat16)
    cos, sin = ops.rope_tables(T, D, device=dev)
    kc = torch.zeros(B, T, Hkv, D, device=dev, dtype=torch.bfloat16)
    vc = torch.zeros_like(kc)
    q = ops.decode_rope_cache(qkv, kc, vc, cos, sin, pos, Hq)
    # CPU fallback on the same inputs
    kc2 = torch.zeros(B, T, Hkv, D, dtype=torch.bfloat16)
    vc2 = torch.zeros_like(kc2)
    q2 = ops.decode_rope_cache(qkv.cpu(), kc2, vc2, cos.cpu(), sin.cpu(),
                               pos, Hq)
    assert torch.allclose(q.cpu().float(), q2.float(), atol=2e-2)
    assert torch.allclose(kc.cpu().float(), kc2.float(), atol=2e-2)
    assert torch.equal(vc.cpu(), vc2)
    # int32 device-scalar position agrees with the host int
    kc3 = torch.zeros_like(kc)
    vc3 = torch.zeros_like(vc)
    p32 = torch.tensor([pos], dtype=torch.int32, device=dev)
    q3 = ops.decode_rope_cache(qkv, kc3, vc3, cos, sin, p32, Hq)
    assert torch.equal(q3, q)
    assert torch.equal(kc3, kc)
    assert torch.equal(vc3, vc)


@pytest.mark.gpu
def test_decode_attention_split_long_cache():
    # L > 512 exercises multi-row-per-wave accumulation in every split
    from torchx_amd import ops
    from torchx_amd.ops import reference

    dev = torch.device("cuda:0")
    torch.manual_seed(8)
    B, Hq, Hkv, T, L, D = 2, 4, 2, 1200, 1101, 128
    q = torch.randn(B, Hq, D, device=dev, dtype=torch.bfloat16)
    kc = torch.randn(B, T, Hkv, D, device=dev, dtype=torch.bfloat16)
    vc = torch.randn(B, T, Hkv, D, device=dev, dtype=torch.bfloat16)
    o = ops.decode_attention(q, kc, vc, L)
    ref = reference.decode_attention(q.cpu(), kc.cpu(), vc.cpu(), L,
                                     1.0 / D ** 0.5)
    err = (o.cpu().float() - ref.float()).abs().max().item()
    assert err < 3e-2, err


@pytest.mark.gpu
@pytest.mark.parametrize("B,Hq,Hkv", [(2, 8, 4),     # B*Hq < 512: split
                                      (8, 64, 8)],   # B*Hq = 512: single pass
                         ids=["split", "single-pass"])
def test_decode_attention_length_paths_bit_identical(B, Hq, Hkv):
    # the host length, the device scalar pos and the per-row [B] pos reach
    # the same kernel body: same L -> same bits. L = 33 leaves the 16-row
    # loop a ragged tail and the split chunks unequal.
    from torchx_amd import ops

    dev = torch.device("cuda:0")
    torch.manual_seed(11)
    T, L, D = 48, 33, 128
    q = torch.randn(B, Hq, D, device=dev, dtype=torch.bfloat16)
    kc = torch.randn(B, T, Hkv, D, device=dev, dtype=torch.bfloat16)
    vc = torch.randn(B, T, Hkv, D, device=dev, dtype=torch.bfloat16)
    o_host = ops.decode_attention(q, kc, vc, L)
    pos1 = torch.tensor([L - 1], device=dev, dtype=torch.int32)
    o_scalar = ops.decode_attention_dev(q, kc, vc, pos1)
    posB = torch.full((B,), L - 1, device=dev, dtype=torch.int32)
    o_rows = ops.decode_attention_dev(q, kc, vc, posB)
    assert torch.equal(o_host, o_scalar)
    assert torch.equal(o_host, o_rows)


def test_generate_app_cpu(capsys):
    from torchx_amd.apps import generate_main

    rc = generate_main.main(["--model", "tiny", "--batch", "2",
                             "--prompt-len", "12", "--new-tokens", "4"])
    assert rc == 0
    import json as _json

    line = capsys.readouterr().out.strip().splitlines()[-1]
    rec = _json.loads(line)
    assert rec["tokens_per_second"] > 0
    assert rec["new_tokens"] == 4


@pytest.mark.gpu
def test_generate_app_gpu_graphed(capsys):
    from torchx_amd.apps import generate_main

    rc = generate_main.main(["--model", "gpu_tiny", "--batch", "2",
                             "--prompt-len", "32", "--new-tokens", "8",
                             "--graph"])
    assert rc == 0


@pytest.mark.gpu
def test_gemv_swiglu_matches_reference():
    from torchx_amd.ops import hip_ops

    dev = torch.device("cuda:0")
    torch.manual_seed(9)
    for M, I, K in [(4, 14336, 4096), (1, 100, 512), (8, 333, 1536)]:
        x = torch.randn(M, K, device=dev, dtype=torch.bfloat16)
        w = torch.randn(2 * I, K, device=dev, dtype=torch.bfloat16)
        out = hip_ops().gemv_swiglu_bf16(x, w)
        gu = x.float() @ w.float().t()
        g, u = gu.chunk(2, dim=-1)
        ref = torch.nn.functional.silu(g) * u
        err = (out.float() - ref).abs().max().item()
        scale = ref.abs().max().item() + 1
        assert err < 2e-2 * K ** 0.5 + 2e-2 * scale, (M, I, K, err)


def test_continuous_batcher_matches_per_sequence():
    """Two prompts of DIFFERENT lengths decoded together in one ragged
    batch must produce exactly the tokens each would get alone (greedy),
    and a retired row re-admitted mid-flight must not disturb others."""
    from torchx_amd.models.generate import ContinuousBatcher

    torch.manual_seed(11)
    cfg = llama_tiny()
    model = LlamaModel(cfg)
    p1 = torch.randint(0, cfg.vocab_size, (11,))
    p2 = torch.randint(0, cfg.vocab_size, (17,))
    p3 = torch.randint(0, cfg.vocab_size, (7,))

    solo = {}
    for name, p in [("p1", p1), ("p2", p2), ("p3", p3)]:
        out = generate(model, p.reshape(1, -1), max_new_tokens=5)
        solo[name] = out[0, p.numel():].tolist()

    cb = ContinuousBatcher(model, max_batch=2, max_len=64)
    t1 = cb.admit(0, p1)
    t2 = cb.admit(1, p2)
    got1, got2 = [int(t1)], [int(t2)]
    for _ in range(4):
        toks = cb.step()
        got1.append(int(toks[0]))
        got2.append(int(toks[1]))
    assert got1 == solo["p1"], (got1, solo["p1"])
    assert got2 == solo["p2"], (got2, solo["p2"])

    # retire row 0, admit p3 there while row 1 keeps decoding
    cb.retire(0)
    assert cb.free_rows() == [0]
    t3 = cb.admit(0, p3)
    got3 = [int(t3)]
    more2 = []
    for _ in range(4):
        toks = cb.step()
        got3.append(int(toks[0]))
        more2.append(int(toks[1]))
    assert got3 == solo["p3"], (got3, solo["p3"])
    # row 1 continues its own stream: tokens 6..9 of a longer solo run
    out2_long = generate(model, p2.reshape(1, -1), max_new_tokens=9)
    assert more2 == out2_long[0, p2.numel() + 5:].tolist()


@pytest.mark.gpu
def test_continuous_batcher_gpu_matches_per_sequence():
    from torchx_amd.models.generate import ContinuousBatcher
    from torchx_amd.models.llama import llama_gpu_tiny

    dev = torch.device("cuda:0")
    torch.manual_seed(12)
    cfg = llama_gpu_tiny()
    model = LlamaModel(cfg, device=dev)
    p1 = torch.randint(0, cfg.vocab_size, (24,), device=dev)
    p2 = torch.randint(0, cfg.vocab_size, (40,), device=dev)
    solo1 = generate(model, p1.reshape(1, -1), 5)[0, 24:].tolist()
    solo2 = generate(model, p2.reshape(1, -1), 5)[0, 40:].tolist()
    cb = ContinuousBatcher(model, max_batch=2, max_len=96)
    got1 = [int(cb.admit(0, p1))]
    got2 = [int(cb.admit(1, p2))]
    for _ in range(4):
        toks = cb.step()
        got1.append(int(toks[0]))
        got2.append(int(toks[1]))
    assert got1 == solo1, (got1, solo1)
    assert got2 == solo2, (got2, solo2)


def test_continuous_batcher_auto_retire():
    """A row that exhausts its cache pool is retired automatically and
    its slot becomes re-admittable."""
    from torchx_amd.models.generate import ContinuousBatcher

    torch.manual_seed(13)
    cfg = llama_tiny()
    model = LlamaModel(cfg)
    cb = ContinuousBatcher(model, max_batch=2, max_len=16)
    cb.admit(0, torch.randint(0, cfg.vocab_size, (12,)))
    assert cb.free_rows() == [1]
    for _ in range(3):
        cb.step()
    assert not cb.active[0]          # pos reached 15: the 16-row pool is up
    assert 0 in cb.free_rows()
    cb.admit(0, torch.randint(0, cfg.vocab_size, (5,)))
    assert cb.active[0]


# ---------------------------------------------------------------------------
# Op-call traces of the serving passes. The expected sequences were recorded
# with this recorder on the per-family passes that preceded the shared ones;
# a change that adds, drops or reorders a dispatch fails here.
# ---------------------------------------------------------------------------

_SERVING_OPS = (
    "rmsnorm", "rope", "flash_attention", "swiglu_packed",
    "paged_prefill_attention", "paged_prefill_rope_cache",
    "paged_prefill_attention_ragged", "rmsnorm_res", "decode_linear",
    "decode_linear_swiglu", "decode_rope_cache", "decode_attention",
    "decode_attention_dev", "paged_decode_rope_cache",
    "paged_decode_attention",
)


def _record_calls(monkeypatch, targets):
    """Wrap ``(owner, name)`` attributes so that every call made from
    outside another wrapped call appends ``name`` to the returned list
    (the CPU fallbacks of some ops call ``ops.rope`` themselves; those
    inner calls are no dispatch of the pass)."""
    calls, depth = [], [0]

    def wrap(name, fn):
        def inner(*args, **kwargs):
            if depth[0] == 0:
                calls.append(name)
            depth[0] += 1
            try:
                return fn(*args, **kwargs)
            finally:
                depth[0] -= 1
        return inner

    for owner, name in targets:
        monkeypatch.setattr(owner, name, wrap(name, getattr(owner, name)))
    return calls


def _trace_passes(model, calls, prefill, prefill_extend, prefill_ragged,
                  decode_step):
    """Run each serving pass once on B = 2 and return its op-call list by
    name: the three prefill kinds, then one decode step per cache kind."""
    from torchx_amd.models.generate import PagedKVCache

    cfg = model.cfg
    cpu = torch.device("cpu")
    B, S, P = 2, 20, 16
    tokens = torch.randint(0, cfg.vocab_size, (B, S))
    table = torch.tensor([[1, 2], [3, 4]], dtype=torch.int32)
    pos = torch.full((B,), S, dtype=torch.int32)

    def dense():
        return [KVCache.empty(cfg, B, 2 * P, cpu)
                for _ in range(cfg.num_layers)]

    def paged():
        return [PagedKVCache.empty(cfg, 5, P, table, cpu)
                for _ in range(cfg.num_layers)]

    def run(fn, *args, **kwargs):
        calls.clear()
        fn(model, *args, **kwargs)
        return list(calls)

    out = {}
    d, pg = dense(), paged()
    out["prefill"] = run(prefill, tokens, d)
    out["prefill_paged"] = run(prefill, tokens, pg)
    out["prefill_extend"] = run(prefill_extend, tokens[:, :7], paged(), 0)
    out["prefill_ragged"] = run(prefill_ragged, tokens.reshape(-1), paged(),
                                [0, 1], [S, S], [0, 0])
    nxt = tokens[:, -1:]
    out["decode_paged"] = run(decode_step, nxt, pg, pos_dev=pos)
    out["decode_rows"] = run(decode_step, nxt, dense(), pos_dev=pos)
    out["decode_dense"] = run(decode_step, nxt, d)
    return out


def _decode_trace(rope_cache, attention, mlp, layers):
    layer = (["decode_linear", rope_cache, attention, "decode_linear",
              "rmsnorm_res"] + mlp + ["rmsnorm_res"])
    return ["rmsnorm_res"] + layers * layer + ["decode_linear"]


def test_serving_passes_op_call_trace(monkeypatch):
    from torchx_amd import ops
    from torchx_amd.models.generate import prefill_extend, prefill_ragged

    torch.manual_seed(20)
    cfg = llama_tiny()
    assert cfg.num_layers == 2
    model = LlamaModel(cfg)
    calls = _record_calls(monkeypatch, [(ops, n) for n in _SERVING_OPS])
    got = _trace_passes(model, calls, prefill, prefill_extend, prefill_ragged,
                        decode_step)

    mlp = ["rmsnorm", "swiglu_packed"]
    dense_prefill = 2 * (["rmsnorm", "rope", "rope", "flash_attention"]
                         + mlp) + ["rmsnorm"]
    assert got["prefill"] == dense_prefill
    assert got["prefill_paged"] == dense_prefill
    assert got["prefill_extend"] == 2 * (
        ["rmsnorm", "rope", "rope", "paged_prefill_attention"] + mlp
    ) + ["rmsnorm"]
    assert got["prefill_ragged"] == 2 * (
        ["rmsnorm", "paged_prefill_rope_cache",
         "paged_prefill_attention_ragged"] + mlp
    ) + ["rmsnorm"]

    mlp = ["decode_linear_swiglu", "decode_linear"]
    want = {
        "decode_dense": _decode_trace("decode_rope_cache",
                                      "decode_attention", mlp, 2),
        "decode_rows": _decode_trace("decode_rope_cache",
                                     "decode_attention_dev", mlp, 2),
        "decode_paged": _decode_trace("paged_decode_rope_cache",
                                      "paged_decode_attention", mlp, 2),
    }
    for kind, trace in want.items():
        assert got[kind] == trace, kind
        # 8 dispatches per layer (docs/kernels.md), the leading norm and
        # the lm_head GEMV
        assert len(got[kind]) == 1 + 8 * cfg.num_layers + 1, kind


@pytest.mark.parametrize("S0", [32, 33], ids=["S0%P==0", "S0%P==1"])
def test_paged_batcher_refused_shared_admit_leaves_nothing(S0):
    """A prompt that shares pages and is refused for lack of pages leaves
    the table, refcounts, index and shared_tokens as they were. At these
    lengths the hit cap ``(S0 - 1) // P`` and the registration range
    ``S0 // P`` differ (or just stop differing)."""
    from torchx_amd.models.generate import OutOfPages, PagedBatcher

    torch.manual_seed(21)
    cfg = llama_tiny()
    model = LlamaModel(cfg)
    P = 16
    head = torch.randint(0, cfg.vocab_size, (33,))
    p0 = torch.cat([head, torch.randint(0, cfg.vocab_size, (5,))])   # 38
    p1 = head[:S0]
    hits = (S0 - 1) // P                  # 1 page at 32, 2 pages at 33
    fresh = -(-(S0 + 1) // P) - hits      # 2 pages at 32, 1 page at 33
    usable = 3 + fresh
    pb = PagedBatcher(model, max_batch=2, max_len=96, num_pages=1 + usable,
                      page_size=P, prefix_sharing=True)
    al = pb.allocator
    pb.admit(0, p0)                       # 3 pages, 2 of them indexed
    assert len(pb._index) == 2 and pb.free_pages() == fresh
    other = al.alloc(1)                   # someone else's page
    table = pb.block_table.clone()
    refs = [al.refcount(p) for p in range(al.num_pages)]
    index, page_key = dict(pb._index), dict(pb._page_key)
    with pytest.raises(OutOfPages):
        pb.admit(1, p1)                   # one page short
    assert torch.equal(pb.block_table, table)
    assert [al.refcount(p) for p in range(al.num_pages)] == refs
    assert pb._index == index and pb._page_key == page_key
    assert pb.shared_tokens == [0, 0] and pb.pages[1] == []
    assert pb.free_rows() == [1] and pb.free_pages() == fresh - 1

    al.free(other)
    first = int(pb.admit(1, p1))
    assert first == int(generate(model, p1.reshape(1, -1), 1)[0, S0])
    assert pb.shared_tokens == [0, hits * P]
    assert pb.pages[1][:hits] == pb.pages[0][:hits]
    assert pb.free_pages() == 0
    # its own second page at S0 = 32 duplicates an indexed key: not indexed
    assert pb._index == index and pb._page_key == page_key
    pb.retire(0)
    pb.retire(1)
    assert pb._index == {} and pb._page_key == {}
    assert pb.free_pages() == usable
    assert all(al.refcount(p) == 0 for p in range(al.num_pages))
