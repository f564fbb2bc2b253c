"""Block maps of the dense attention forward: "balanced" (and its
tiles-ascending variant "adjacent") must give the bits of "legacy" — the
map only reorders which block computes which (batch, head, q tile) — and
stay within the fp32-reference tolerance of tests/test_ops_gpu.py."""

import math

import pytest
import torch

from torchx_amd import ops
from torchx_amd.ops import reference

pytestmark = pytest.mark.gpu

# (B, Hq, Hkv, S)
SHAPES = [
    (2, 8, 4, 384),    # B*Hkv = 8: the XCD path, nqt = 3
    (1, 8, 2, 256),    # B*Hkv = 2: the fallback path (rounded-up grid)
    (3, 8, 8, 200),    # 24 streams, ragged last tile
    (4, 32, 8, 512),
]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture()
def restore_map():
    before = ops.get_attn_fwd_map()
    yield
    ops.set_attn_fwd_map(before)


def rel_err(a, b):
    a, b = a.float(), b.float()
    return (a - b).abs().max().item() / (b.abs().max().item() + 1e-6)


@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("B,Hq,Hkv,S", SHAPES)
def test_balanced_map_bits_equal_legacy(dev, restore_map, B, Hq, Hkv, S,
                                        causal):
    D = 128
    g = torch.Generator(device="cpu").manual_seed(B * 1000 + S)
    q, k, v = (torch.randn(B, S, h, D, generator=g).to(torch.bfloat16).to(dev)
               for h in (Hq, Hkv, Hkv))
    scale = 1.0 / math.sqrt(D)
    out = {}
    for name in ("legacy", "balanced", "adjacent"):
        ops.set_attn_fwd_map(name)
        assert ops.get_attn_fwd_map() == name
        o, lse = ops.hip_ops().attn_fwd(q, k, v, scale, causal)
        out[name] = (o.clone(), lse.clone())
        # the allocator hands the next call this storage again: poison it,
        # so a tile the next map leaves unwritten shows up as NaN
        o.fill_(float("nan"))
        lse.fill_(float("nan"))
    for name in ("balanced", "adjacent"):
        assert torch.equal(out[name][0], out["legacy"][0]), name
        assert torch.equal(out[name][1], out["legacy"][1]), name

    o_ref = reference.attention(q, k, v, causal=causal)
    lse_ref = reference.attention_lse(q, k, v, causal=causal)
    for name in ("legacy", "balanced"):
        assert rel_err(out[name][0], o_ref) < 3e-2, name
        assert rel_err(out[name][1], lse_ref) < 2e-2, name


def test_set_attn_fwd_map_round_trip(dev, restore_map):
    for name in ("legacy", "balanced", "adjacent", "balanced"):
        ops.set_attn_fwd_map(name)
        assert ops.get_attn_fwd_map() == name
    with pytest.raises(RuntimeError):
        ops.set_attn_fwd_map("heaviest")
    with pytest.raises(RuntimeError):
        ops.set_attn_fwd_map("")
    assert ops.get_attn_fwd_map() == "balanced"
