"""Mixtral serving path: cached MoE decode must agree with a full
re-forward (CPU reference kernels here, HIP kernels in the gpu test)."""

import pytest
import torch

from torchx_amd.models.generate_moe import (
    KVCache, decode_step_moe, generate_moe, prefill_moe,
)
from torchx_amd.models.mixtral import MixtralModel, mixtral_tiny


def test_cached_moe_decode_matches_full_forward():
    torch.manual_seed(0)
    cfg = mixtral_tiny()
    model = MixtralModel(cfg)
    B, S0 = 2, 12
    tokens = torch.randint(0, cfg.vocab_size, (B, S0))
    caches = [KVCache.empty(cfg, B, S0 + 6, torch.device("cpu"))
              for _ in range(cfg.num_layers)]
    pre = prefill_moe(model, tokens, caches)
    with torch.no_grad():
        full = model(tokens)[:, -1]
    assert torch.allclose(pre.float(), full.float(), atol=3e-2), (
        (pre - full).abs().max())

    cur = tokens
    nxt = pre.argmax(-1, keepdim=True)
    for _ in range(3):
        dec = decode_step_moe(model, nxt, caches)
        cur = torch.cat([cur, nxt], dim=1)
        with torch.no_grad():
            full = model(cur)[:, -1]
        assert torch.allclose(dec.float(), full.float(), atol=4e-2), (
            (dec - full).abs().max())
        nxt = dec.argmax(-1, keepdim=True)


def test_generate_moe_shapes():
    torch.manual_seed(1)
    cfg = mixtral_tiny()
    model = MixtralModel(cfg)
    tokens = torch.randint(0, cfg.vocab_size, (2, 8))
    out = generate_moe(model, tokens, max_new_tokens=4)
    assert out.shape == (2, 12)
    assert torch.equal(out[:, :8], tokens)
    out2 = generate_moe(model, tokens, max_new_tokens=4)
    assert torch.equal(out, out2)  # greedy determinism
    out3 = generate_moe(model, tokens, max_new_tokens=3, temperature=0.7,
                        top_k=10)
    assert out3.shape == (2, 11)


@pytest.mark.gpu
def test_generate_moe_gpu_end_to_end():
    from torchx_amd.models.mixtral import mixtral_gpu_tiny

    dev = torch.device("cuda:0")
    torch.manual_seed(2)
    cfg = mixtral_gpu_tiny()
    model = MixtralModel(cfg, device=dev)
    tokens = torch.randint(0, cfg.vocab_size, (2, 32), device=dev)
    out = generate_moe(model, tokens, max_new_tokens=6)
    assert out.shape == (2, 38)
    # cached decode logits agree with a full re-forward on the HIP path
    caches = [KVCache.empty(cfg, 2, 48, dev) for _ in range(cfg.num_layers)]
    prefill_moe(model, tokens, caches)
    nxt = tokens[:, -1:]
    dec = decode_step_moe(model, nxt, caches)
    with torch.no_grad():
        full = model(torch.cat([tokens, nxt], 1))[:, -1]
    err = (dec.float() - full.float()).abs().max().item()
    scale = full.float().abs().max().item() + 1e-6
    assert err < 5e-2 * scale, (err, scale)


def test_generate_app_moe_cpu(capsys):
    from torchx_amd.apps import generate_main

    rc = generate_main.main(["--model", "mixtral_tiny", "--batch", "2",
                             "--prompt-len", "10", "--new-tokens", "3"])
    assert rc == 0
    import json as _json

    rec = _json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert rec["model"] == "mixtral_tiny" and rec["tokens_per_second"] > 0
    # --graph is refused for MoE models
    rc = generate_main.main(["--model", "mixtral_tiny", "--graph",
                             "--prompt-len", "8", "--new-tokens", "2"])
    assert rc == 1


def test_continuous_batcher_moe_matches_per_sequence():
    """Ragged MoE decode: two Mixtral prompts of different lengths in one
    batcher produce exactly their solo greedy streams."""
    from torchx_amd.models.generate import ContinuousBatcher

    torch.manual_seed(14)
    cfg = mixtral_tiny()
    model = MixtralModel(cfg)
    p1 = torch.randint(0, cfg.vocab_size, (9,))
    p2 = torch.randint(0, cfg.vocab_size, (14,))
    solo1 = generate_moe(model, p1.reshape(1, -1), 4)[0, 9:].tolist()
    solo2 = generate_moe(model, p2.reshape(1, -1), 4)[0, 14:].tolist()
    cb = ContinuousBatcher(model, max_batch=2, max_len=32,
                           prefill_fn=prefill_moe,
                           decode_fn=decode_step_moe)
    got1 = [int(cb.admit(0, p1))]
    got2 = [int(cb.admit(1, p2))]
    for _ in range(3):
        toks = cb.step()
        got1.append(int(toks[0]))
        got2.append(int(toks[1]))
    assert got1 == solo1, (got1, solo1)
    assert got2 == solo2, (got2, solo2)


def test_moe_names_are_aliases_of_the_shared_passes():
    from torchx_amd.models import generate, generate_moe

    assert generate_moe.prefill_moe is generate.prefill
    assert generate_moe.prefill_extend_moe is generate.prefill_extend
    assert generate_moe.prefill_ragged_moe is generate.prefill_ragged
    assert generate_moe.decode_step_moe is generate.decode_step
    assert generate_moe.generate_moe is generate.generate


def test_moe_serving_passes_op_call_trace(monkeypatch):
    """Mixtral counterpart of test_generate's trace: the attention half
    dispatches as Llama's does; the MLP half is one ``swiglu_packed`` per
    expert in prefill and one ``_moe_mlp_decode`` (its expert GEMVs depend
    on the routing, so it is traced as a unit) in decode."""
    from test_generate import (
        _SERVING_OPS, _decode_trace, _record_calls, _trace_passes,
    )
    from torchx_amd import ops
    from torchx_amd.models import generate_moe

    torch.manual_seed(22)
    cfg = mixtral_tiny()
    assert cfg.num_layers == 2 and cfg.num_experts == 4
    model = MixtralModel(cfg)
    calls = _record_calls(
        monkeypatch, [(ops, n) for n in _SERVING_OPS]
        + [(generate_moe, "_moe_mlp_decode")])
    got = _trace_passes(model, calls, prefill_moe,
                        generate_moe.prefill_extend_moe,
                        generate_moe.prefill_ragged_moe, decode_step_moe)

    mlp = ["rmsnorm"] + 4 * ["swiglu_packed"]
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

    mlp = ["_moe_mlp_decode"]
    assert got["decode_dense"] == _decode_trace(
        "decode_rope_cache", "decode_attention", mlp, 2)
    assert got["decode_rows"] == _decode_trace(
        "decode_rope_cache", "decode_attention_dev", mlp, 2)
    assert got["decode_paged"] == _decode_trace(
        "paged_decode_rope_cache", "paged_decode_attention", mlp, 2)


def _serve_two(make, many):
    """Admit two prompts into the batcher ``make()`` builds, step 6 times;
    returns (batcher, first tokens + every step's tokens)."""
    b = make()
    torch.manual_seed(23)
    vocab = b.cfg.vocab_size
    head = torch.randint(0, vocab, (20,))
    p1 = torch.cat([head, torch.randint(0, vocab, (3,))])
    p2 = torch.cat([head, torch.randint(0, vocab, (10,))])
    if many:
        out = [b.admit_many([0, 1], [p1, p2]).tolist()]
    else:
        out = [[int(b.admit(0, p1)), int(b.admit(1, p2))]]
    for _ in range(6):
        out.append(b.step().tolist())
    return b, out


def test_mixtral_batchers_need_no_function_arguments():
    """Batchers built with no ``*_fn`` run a Mixtral model exactly as ones
    given the four ``*_moe`` functions do."""
    from torchx_amd.models import generate_moe as gm
    from torchx_amd.models.generate import ContinuousBatcher, PagedBatcher

    torch.manual_seed(24)
    model = MixtralModel(mixtral_tiny())
    dense_fns = dict(prefill_fn=gm.prefill_moe, decode_fn=gm.decode_step_moe)
    paged_fns = dict(extend_fn=gm.prefill_extend_moe,
                     ragged_fn=gm.prefill_ragged_moe, **dense_fns)

    def paged(**fns):
        return PagedBatcher(model, max_batch=2, max_len=64, num_pages=8,
                            page_size=16, prefix_sharing=True,
                            prefill_chunk=7, **fns)

    def dense(**fns):
        return ContinuousBatcher(model, max_batch=2, max_len=64, **fns)

    _, want_dense = _serve_two(lambda: dense(**dense_fns), many=False)
    _, got_dense = _serve_two(dense, many=False)
    assert got_dense == want_dense
    for many in (False, True):
        want_pb, want = _serve_two(lambda: paged(**paged_fns), many)
        got_pb, got = _serve_two(paged, many)
        assert got == want == want_dense, many
        assert got_pb.shared_tokens == want_pb.shared_tokens == [0, 16]
        assert got_pb.pages == want_pb.pages
        assert torch.equal(got_pb.block_table, want_pb.block_table)


@pytest.mark.gpu
def test_paged_batcher_mixtral_defaults_gpu_admit_many_matches_admit():
    """Default functions on the HIP path: a multi-tile, a sub-tile and a
    single-row prompt give the same first and next 4 tokens whether they
    are admitted one by one or packed."""
    from torchx_amd.models.generate import PagedBatcher
    from torchx_amd.models.mixtral import mixtral_gpu_tiny

    dev = torch.device("cuda:0")
    torch.manual_seed(25)
    cfg = mixtral_gpu_tiny()
    model = MixtralModel(cfg, device=dev)
    prompts = [torch.randint(0, cfg.vocab_size, (n,), device=dev)
               for n in (130, 17, 1)]
    streams = []
    for many in (False, True):
        pb = PagedBatcher(model, max_batch=3, max_len=160, num_pages=16,
                          page_size=16)
        if many:
            out = [pb.admit_many([0, 1, 2], prompts).tolist()]
        else:
            out = [[int(pb.admit(r, p)) for r, p in enumerate(prompts)]]
        for _ in range(4):
            out.append(pb.step().tolist())
        streams.append(out)
    assert streams[0] == streams[1], streams
