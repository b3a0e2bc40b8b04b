"""The wide MoE dispatch (moe_wide.hip: 128 experts, top-k <= 8) on the GPU: exact routing probes in
both K-loop forms, the placement's layout, and the whole block against an fp32 per-expert reference."""
import pytest
import torch

from mlopamd import ops
from mlopamd.ops import reference as ref

pytestmark = pytest.mark.gpu
bf = torch.bfloat16
E = 128


def _probe(T, H, gpu):
    """x rows: 32 entries of +-1; router entries {-1, 0, 1} / 8: every logit is a multiple of 1/8 with
    |logit| <= 4, exact in fp32 in any order and in bf16, with many ties.  Row T - 1 (T >= 5): all logits equal."""
    g = torch.Generator().manual_seed(1000 * T + H)
    x = torch.zeros(T, H)
    for t in range(T):
        cols = torch.randperm(H, generator=g)[:32]
        x[t, cols] = torch.randint(0, 2, (32,), generator=g).float() * 2 - 1
    if T >= 5:
        x[T - 1] = 0
    wr = torch.randint(-1, 2, (E, H), generator=g).float() / 8
    logits = (x.double() @ wr.double().t())
    return x.to(gpu, bf), wr.to(gpu, bf), logits.to(gpu)


@pytest.mark.parametrize("renorm", [True, False])
@pytest.mark.parametrize("k", [1, 8])
@pytest.mark.parametrize("H", [256, 2048])
@pytest.mark.parametrize("T", [1, 5, 16, 17, 64, 65, 200])  # <= 16: K-split form; then 64-token tiles
def test_route_wide_exact(gpu, T, H, k, renorm):
    _check_route(gpu, T, H, k, renorm)


@pytest.mark.parametrize("T,H", [(3, 128), (16, 384), (70, 160)])  # one K step per wave; a ring tail; a half slab
def test_route_wide_exact_k_loop_edges(gpu, T, H):
    _check_route(gpu, T, H, 8, True)


def _check_route(gpu, T, H, k, renorm):
    x, wr, logits = _probe(T, H, gpu)
    assert float(logits.abs().max()) <= 4 and bool((logits * 8 == (logits * 8).round()).all())
    topw, topi = ops.moe_route_wide(x, wr, k, renorm)
    _, i_ref = ref.moe_route(logits, k)
    assert torch.equal(topi, i_ref)  # every token: ties go to the lower id
    if T >= 5:
        assert topi[T - 1].tolist() == list(range(k))
    w_ref = torch.softmax(logits, -1).gather(1, i_ref.long())
    if renorm:
        w_ref = w_ref / w_ref.sum(-1, keepdim=True)
    err = float(((topw.double() - w_ref).abs() / w_ref).max())
    print(f"T={T} H={H} k={k} renorm={renorm}: max relative weight error {err:.3g}")
    # (128 + 8) x 2^-24 for the two sums plus ~1e-6 per exp, doubled
    torch.testing.assert_close(topw.double(), w_ref, rtol=2e-5, atol=0)


@pytest.mark.parametrize("e0,n_local", [(0, 128), (32, 64)])
@pytest.mark.parametrize("T", [5, 200])
def test_place_wide_layout(gpu, T, e0, n_local):
    k = 8
    x, wr, _ = _probe(T, 256, gpu)
    topw, topi, xs, offsets, arow, inv = ops.moe_dispatch_wide(x, wr, k, e0, n_local)
    assert xs.data_ptr() == x.data_ptr()  # no gathered copy
    loc = topi.reshape(-1).long() - e0
    ok = (loc >= 0) & (loc < n_local)
    counts = torch.bincount(loc[ok], minlength=n_local)
    assert offsets.tolist() == [0, *torch.cumsum(counts, 0).tolist()]
    assert torch.equal(inv < 0, ~ok)
    slots = torch.nonzero(ok).view(-1)
    assert torch.equal(arow[inv[slots].long()].long(), slots // k)
    off = offsets.tolist()
    for e in range(n_local):
        got = sorted(arow[off[e]:off[e + 1]].tolist())
        assert got == sorted((slots[loc[slots] == e] // k).tolist()), e


@pytest.fixture(scope="module")
def block_weights(gpu):
    H, I = 2048, 768
    torch.manual_seed(7)
    return ((0.05 * torch.randn(E, H, device=gpu)).to(bf), (0.03 * torch.randn(E, 2 * I, H, device=gpu)).to(bf),
            (0.03 * torch.randn(E, H, I, device=gpu)).to(bf), (1 + 0.1 * torch.randn(H, device=gpu)).to(bf))


@pytest.mark.parametrize("T", [8, 96])
def test_moe_block_wide_dispatch_matches_fp32(gpu, block_weights, T):
    """The whole block against the fp32 per-expert reference on the kernel's own routing
    (test_moe_block_mid_dispatch_matches_fp32's tolerance)."""
    from mlopamd.parallel import moe as moe_mod

    wr, w13, w2, nw = block_weights
    k, H = 8, 2048
    torch.manual_seed(T)
    x = torch.randn(T, H, device=gpu, dtype=bf)
    res = torch.randn(T, H, device=gpu, dtype=bf)
    topw, topi = ops.moe_route_wide(x, wr, k)
    r2 = res.clone()
    out = moe_mod.moe_forward_add_norm(x, wr, w13, w2, k, 0, E, r2, nw, 1e-6)
    y = torch.zeros(T, H, device=gpu)
    for t in range(T):
        for j in range(k):
            e = int(topi[t, j])
            gu = x[t].float() @ w13[e].float().t()
            h = ref.silu_mul(ops.deinterleave_cols(gu.to(bf).view(1, -1))).float().view(-1)
            y[t] += topw[t, j] * (h.to(bf).float() @ w2[e].float().t())
    exp_out, exp_res = ref.add_rmsnorm(y.to(bf), res, nw, 1e-6)
    torch.testing.assert_close(r2, exp_res, atol=3e-2, rtol=3e-2)
    torch.testing.assert_close(out, exp_out, atol=5e-2, rtol=5e-2)
