"""gemm_mx4t.hip (the fused tiled MXFP4 GEMM) on the GPU: an exact layout probe, ops/reference.py's
fp64 ``gemm_mx4`` under test_mx4_kernels_gpu.py's derived bound, the fused SiLU-mul against the plain
launch, and the routing of ``ops.gemm_mx4``.  Scale bytes as there: [2, 252] for the exact tests."""
import pytest
import torch

from mlopamd import ops
from mlopamd.ops import reference as ref

pytestmark = pytest.mark.gpu
SHAPES = [(128, 128), (256, 640), (384, 1792)]  # one K tile; 5 (uneven splits, tail only); 14 (steady loop)
ROWS = [1, 17, 64, 65, 128, 129, 200]           # MT = 2, 2, 4, 8, 8 and two M-tiles (1 and 72 rows in the last)


def _weights(N, K, dev, seed, e_lo, e_hi):
    """Random codes over all 16 values and random scale bytes in [e_lo, e_hi], packed."""
    g = torch.Generator(device=dev).manual_seed(seed)
    codes = torch.randint(0, 16, (N, K), generator=g, device=dev, dtype=torch.uint8)
    e = torch.randint(e_lo, e_hi + 1, (N, K // 32), generator=g, device=dev, dtype=torch.uint8)
    return codes, e, ops.mx4_pack(codes, e)


def _tile(x, W, epi=ops.EPI_NONE, ks=0, pad=0):
    out = torch.full((x.shape[0] + pad, W.N // 2 if epi else W.N), 7.0, device=x.device, dtype=torch.bfloat16)
    torch.ops.mlop.gemm_mx4_tile(out[: x.shape[0]], x, W.qw, W.qe, W.N, epi, ks)
    return out


def _ulp(v):
    return torch.ldexp(torch.ones_like(v), torch.frexp(v)[1] - 8)


@pytest.mark.parametrize("ks", [1, 2, 4])
@pytest.mark.parametrize("c", range(8))
def test_mx4_tile_layout_probe(gpu, monkeypatch, c, ks):
    """x[m, (8 m + c) % K] = 1: output row m is that column of the dequantised weight, exactly (a
    one-hot sum is exact in any order): every lane, byte select, wave-to-row-block map, the LDS image
    of A, the ragged second M-tile (2 rows) and the split boundaries."""
    N, K, M = 256, 512, 130
    codes, e, _ = _weights(N, K, gpu, c, 2, 252)
    e.view(-1)[:4] = torch.tensor([2, 3, 251, 252], dtype=torch.uint8, device=gpu)   # both ends, always
    W = ops.mx4_pack(codes, e)
    cols = (8 * torch.arange(M, device=gpu) + c) % K
    x = torch.zeros(M, K, device=gpu, dtype=torch.bfloat16)
    x[torch.arange(M, device=gpu), cols] = 1
    want = ref.mx4_dequant(codes, e)[:, cols].T
    assert torch.equal(_tile(x, W, ks=ks), want)
    monkeypatch.setattr(ops, "MX4_TILE_MAX_M", 256)
    assert torch.equal(ops.gemm_mx4(x, W), want)


@pytest.mark.parametrize("split", [False, True], ids=["ks-auto", "ks-max"])
@pytest.mark.parametrize("M", ROWS)
@pytest.mark.parametrize("N,K", SHAPES)
def test_gemm_mx4_tile_vs_fp64(gpu, M, N, K, split):
    """The launcher's split and the largest feasible one (a K tile per split).
    |out - ref| <= 2^-8 |ref| (one bf16 rounding) + K 2^-24 sum_k |w x| (the worst-case fp32
    accumulation bound, any summation order); rows past M keep their sentinel; a relaunch is
    bit-identical."""
    codes, e, W = _weights(N, K, gpu, M * 7 + N, 120, 130)
    x = torch.randn(M, K, device=gpu, dtype=torch.bfloat16)
    ks = K // 128 if split else 0
    out = _tile(x, W, ks=ks, pad=3)
    exp = ref.gemm_mx4(x, codes, e)
    mag = x.double().abs() @ ref.mx4_dequant(codes, e).double().abs().T
    err = (out[:M].double() - exp).abs()
    bound = 2.0 ** -8 * exp.abs() + K * 2.0 ** -24 * mag
    print(f"worst error / bound {float((err / bound.clamp_min(1e-30)).max()):.3f}")
    assert bool((err <= bound).all())
    assert bool((out[M:] == 7.0).all())
    assert torch.equal(_tile(x, W, ks=ks)[:M], out[:M])


@pytest.mark.parametrize("split", [False, True], ids=["ks1", "ks-max"])
@pytest.mark.parametrize("M", ROWS)
@pytest.mark.parametrize("N,K", SHAPES)
def test_mx4_tile_silu_mul_rounds_as_the_plain_launch(gpu, M, N, K, split):
    """The fused epilogue (in the tile kernel at ks = 1, in the reduce kernel above) rounds gate and up
    to bf16 as the plain launch stores them, then is ref.silu_mul of those within one bf16 ulp of the
    silu and one of the product (test_moe_mx4_kernels_gpu.py's criterion for moe_mx4.hip's epilogue)."""
    _codes, _e, W = _weights(N, K, gpu, M * 5 + N, 120, 130)
    x = torch.randn(M, K, device=gpu, dtype=torch.bfloat16)
    ks = max(2, K // 128) if split else 1
    if ks > K // 128:
        with pytest.raises(RuntimeError, match="ks"):  # an infeasible forced split is refused
            _tile(x, W, ops.EPI_SILU_MUL, ks)
        return
    y = ops.deinterleave_cols(_tile(x, W, ks=ks)[:M])
    s, u, want = torch.nn.functional.silu(y[:, : N // 2].float()).to(y.dtype).float(), y[:, N // 2:].float(), ref.silu_mul(y).float()
    out = _tile(x, W, ops.EPI_SILU_MUL, ks, pad=3)
    assert bool(((out[:M].float() - want).abs() <= u.abs() * _ulp(s) + _ulp(want)).all())
    assert bool((out[M:] == 7.0).all())


@pytest.mark.parametrize("epi", [ops.EPI_NONE, ops.EPI_SILU_MUL])
def test_mx4_tile_split_under_graph_capture(gpu, epi):
    """A split launch allocates its fp32 partials per call: captured, every replay (with new
    activations in the captured buffer) equals the eager launch."""
    _c, _e, W = _weights(256, 640, gpu, 3, 120, 130)
    x = torch.randn(72, 640, device=gpu, dtype=torch.bfloat16)
    out = torch.empty(72, 128 if epi else 256, device=gpu, dtype=torch.bfloat16)
    torch.ops.mlop.gemm_mx4_tile(out, x, W.qw, W.qe, W.N, epi, 5)  # warm-up outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        torch.ops.mlop.gemm_mx4_tile(out, x, W.qw, W.qe, W.N, epi, 5)
    for seed in range(3):
        x.copy_(torch.randn(72, 640, generator=torch.Generator(device=gpu).manual_seed(seed), device=gpu))
        graph.replay()
        assert torch.equal(out, _tile(x, W, epi, 5)), seed


def test_gemm_mx4_routing(gpu, monkeypatch):
    """Above the streaming kernel's rows ops.gemm_mx4 is the tiled op up to MX4_TILE_MAX_M where the
    shape fits it, and the dequantise + GEMM route otherwise and with the knob at 0."""
    _c, _e, W = _weights(256, 512, gpu, 1, 120, 130)
    _c, _e, W48 = _weights(48, 512, gpu, 2, 120, 130)
    monkeypatch.setattr(ops, "MX4_TILE_MAX_M", 256)
    for M in (65, 200):
        x = torch.randn(M, 512, device=gpu, dtype=torch.bfloat16)
        assert torch.equal(ops.gemm_mx4(x, W), _tile(x, W))
        assert torch.equal(ops.gemm_mx4(x, W, epi=ops.EPI_SILU_MUL), _tile(x, W, ops.EPI_SILU_MUL))
        assert torch.equal(ops.gemm_mx4(x, W48), ops.gemm(x, ops.mx4_dequant(W48)))
    x = torch.randn(65, 512, device=gpu, dtype=torch.bfloat16)
    assert torch.equal(ops.gemm_mx4(torch.cat([x] * 4), W), ops.gemm(torch.cat([x] * 4), ops.mx4_dequant(W)))  # 260 rows
    monkeypatch.setattr(ops, "MX4_TILE_MAX_M", 0)
    assert torch.equal(ops.gemm_mx4(x, W), ops.gemm(x, ops.mx4_dequant(W)))
