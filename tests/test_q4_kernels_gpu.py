"""gemm_q4.hip on the GPU: the int4 weight-streaming MFMA GEMM and the dequantiser against
ops/reference.py's definitions (``gemm_q4`` in fp64, ``q4_dequant`` bit for bit), and the
dequantise-then-GEMM route of ``ops.gemm_q4`` above 64 rows."""
import pytest
import torch

from mlopamd import ops
from mlopamd.ops import reference as ref

pytestmark = pytest.mark.gpu
SHAPES = [(32, 128), (48, 640), (256, 1792), (6144, 4096)]  # 3 idle waves; uneven split, RB = 1; ...


def _weights(N, K, dev, seed):
    """Random q over all 16 values and random normal bf16 scales, packed."""
    g = torch.Generator(device=dev).manual_seed(seed)
    q = torch.randint(-8, 8, (N, K), generator=g, device=dev, dtype=torch.int8)
    s = torch.randn(N, K // 128, generator=g, device=dev).to(torch.bfloat16)
    return q, s, ops.q4_pack(q, s)


@pytest.mark.parametrize("c", range(8))
def test_q4_layout_probe(gpu, c):
    """x[m, 8 m + c] = 1: output row m is column 8 m + c of the dequantised weight, exactly.  The
    eight cases touch every k, all four waves and every lane chunk."""
    N, K, M = 64, 512, 64
    q, s, W = _weights(N, K, gpu, c)
    cols = 8 * torch.arange(M, device=gpu) + c
    x = torch.zeros(M, K, device=gpu, dtype=torch.bfloat16)
    x[torch.arange(M, device=gpu), cols] = 1
    want = ref.q4_dequant(q, s)[:, cols].T
    assert torch.equal(ops.gemm_q4(x, W), want)                             # row blocks per workgroup by N: 1
    for rb in (2, 4):
        out = torch.empty(M, N, device=gpu, dtype=torch.bfloat16)
        torch.ops.mlop.gemm_q4(out, x, W[0], W[1], N, rb)
        assert torch.equal(out, want), rb


@pytest.mark.parametrize("wide", [False, True], ids=["rb-auto", "rb-max"])
@pytest.mark.parametrize("M", [1, 5, 16, 17, 64])
@pytest.mark.parametrize("N,K", SHAPES)
def test_gemm_q4_vs_fp64(gpu, M, N, K, wide):
    """Row blocks per workgroup chosen by N, and the largest of 4 / 2 / 1 with 16 RB | N.
    |out - ref| <= 2^-8 |ref| (one bf16 rounding) + K 2^-24 sum_k |s q x| (the worst-case fp32
    accumulation bound); rows past M keep their sentinel; a relaunch is bit-identical."""
    q, s, W = _weights(N, K, gpu, M * 7 + N)
    x = torch.randn(M, K, device=gpu, dtype=torch.bfloat16)
    rb = (4 if N % 64 == 0 else 2 if N % 32 == 0 else 1) if wide else 0
    out = torch.full((M + 3, N), 7.0, device=gpu, dtype=torch.bfloat16)
    torch.ops.mlop.gemm_q4(out[:M], x, W[0], W[1], N, rb)
    exp = ref.gemm_q4(x, q, s).double()
    mag = x.double().abs() @ (s.double().repeat_interleave(128, 1) * q.double()).abs().T
    err = (out[:M].double() - exp).abs()
    bound = 2.0 ** -8 * exp.abs() + K * 2.0 ** -24 * mag
    print(f"worst error / bound {float((err / bound.clamp_min(1e-30)).max()):.3f}")
    assert bool((err <= bound).all())
    assert bool((out[M:] == 7.0).all())
    out2 = torch.empty_like(out[:M])
    torch.ops.mlop.gemm_q4(out2, x, W[0], W[1], N, rb)
    assert torch.equal(out2, out[:M])


@pytest.mark.parametrize("N,K", SHAPES)
def test_q4_dequant_bit_equal(gpu, N, K):
    q, s, W = _weights(N, K, gpu, N + K)
    assert torch.equal(ops.q4_dequant(W), ref.q4_dequant(q, s))


@pytest.mark.parametrize("epi", [ops.EPI_NONE, ops.EPI_SILU_MUL])
@pytest.mark.parametrize("M", [65, 200])
def test_gemm_q4_large_m_route(gpu, M, epi):
    """Above 64 rows: dequantise into the scratch, then the unchanged bf16 GEMM (its tolerance)."""
    N, K = 1024, 512
    g = torch.Generator(device=gpu).manual_seed(M)
    q, s = ref.q4_quantize((0.02 * torch.randn(N, K, generator=g, device=gpu)).to(torch.bfloat16))
    x = torch.randn(M, K, generator=g, device=gpu).to(torch.bfloat16)
    out = ops.gemm_q4(x, ops.q4_pack(q, s), epi=epi)
    exp = x.float() @ ref.q4_dequant(q, s).float().T
    if epi:
        exp = ref.silu_mul(ops.deinterleave_cols(exp.to(torch.bfloat16))).float()
    torch.testing.assert_close(out.float(), exp, atol=2e-2 * exp.abs().max().item() / 4 + 1e-2, rtol=2e-2)
