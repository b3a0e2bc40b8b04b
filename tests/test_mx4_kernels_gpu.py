"""gemm_mx4.hip on the GPU against ops/reference.py (``gemm_mx4`` in fp64, ``mx4_dequant`` bit for
bit), and the dequantise-then-GEMM route above 64 rows.  The exact tests draw scale bytes from
[2, 252]: at 253 / 254 a weight of 4 x 2^126 is infinite in bf16 (a NaN against a zero activation);
``mx4_quantize`` never produces them."""
import pytest
import torch

from mlopamd import ops
from mlopamd.ops import reference as ref

pytestmark = pytest.mark.gpu
SHAPES = [(32, 128), (48, 640), (256, 1792), (6144, 4096)]  # 3 idle waves; uneven split, RB = 1; ...


def _weights(N, K, dev, seed, e_lo, e_hi):
    """Random codes over all 16 values and random scale bytes in [e_lo, e_hi], packed."""
    g = torch.Generator(device=dev).manual_seed(seed)
    codes = torch.randint(0, 16, (N, K), generator=g, device=dev, dtype=torch.uint8)
    e = torch.randint(e_lo, e_hi + 1, (N, K // 32), generator=g, device=dev, dtype=torch.uint8)
    return codes, e, ops.mx4_pack(codes, e)


@pytest.mark.parametrize("c", range(8))
def test_mx4_layout_probe(gpu, c):
    """x[m, 8 m + c] = 1: output row m is column 8 m + c of the dequantised weight, exactly: every k,
    wave, lane chunk, byte select, code and scale byte; a conversion that rounds or flushes fails."""
    N, K, M = 64, 512, 64
    codes, e, _ = _weights(N, K, gpu, c, 2, 252)
    e.view(-1)[:4] = torch.tensor([2, 3, 251, 252], dtype=torch.uint8, device=gpu)   # both ends, always
    W = ops.mx4_pack(codes, e)
    cols = 8 * torch.arange(M, device=gpu) + c
    x = torch.zeros(M, K, device=gpu, dtype=torch.bfloat16)
    x[torch.arange(M, device=gpu), cols] = 1
    want = ref.mx4_dequant(codes, e)[:, cols].T
    assert torch.equal(ops.gemm_mx4(x, W), want)                            # row blocks per workgroup by N
    for rb in (1, 2, 4):
        out = torch.empty(M, N, device=gpu, dtype=torch.bfloat16)
        torch.ops.mlop.gemm_mx4(out, x, W.qw, W.qe, N, rb)
        assert torch.equal(out, want), rb


@pytest.mark.parametrize("wide", [False, True], ids=["rb-auto", "rb-max"])
@pytest.mark.parametrize("M", [1, 5, 16, 17, 33, 64])
@pytest.mark.parametrize("N,K", SHAPES)
def test_gemm_mx4_vs_fp64(gpu, M, N, K, wide):
    """Row blocks per workgroup chosen by the launcher, and the largest of 4 / 2 / 1 with 16 RB | N.
    |out - ref| <= 2^-8 |ref| (one bf16 rounding) + K 2^-24 sum_k |w x| (the worst-case fp32
    accumulation bound); rows past M keep their sentinel; a relaunch is bit-identical."""
    codes, e, W = _weights(N, K, gpu, M * 7 + N, 120, 130)
    x = torch.randn(M, K, device=gpu, dtype=torch.bfloat16)
    rb = (4 if N % 64 == 0 else 2 if N % 32 == 0 else 1) if wide else 0
    out = torch.full((M + 3, N), 7.0, device=gpu, dtype=torch.bfloat16)
    torch.ops.mlop.gemm_mx4(out[:M], x, W.qw, W.qe, N, rb)
    exp = ref.gemm_mx4(x, codes, e)
    mag = x.double().abs() @ ref.mx4_dequant(codes, e).double().abs().T
    err = (out[:M].double() - exp).abs()
    bound = 2.0 ** -8 * exp.abs() + K * 2.0 ** -24 * mag
    print(f"worst error / bound {float((err / bound.clamp_min(1e-30)).max()):.3f}")
    assert bool((err <= bound).all())
    assert bool((out[M:] == 7.0).all())
    out2 = torch.empty_like(out[:M])
    torch.ops.mlop.gemm_mx4(out2, x, W.qw, W.qe, N, rb)
    assert torch.equal(out2, out[:M])


@pytest.mark.parametrize("N,K", SHAPES)
def test_mx4_dequant_bit_equal(gpu, N, K):
    codes, e, W = _weights(N, K, gpu, N + K, 2, 252)
    assert torch.equal(ops.mx4_dequant(W), ref.mx4_dequant(codes, e))


@pytest.mark.parametrize("epi", [ops.EPI_NONE, ops.EPI_SILU_MUL])
@pytest.mark.parametrize("M", [65, 200])
def test_gemm_mx4_large_m_route(gpu, M, epi):
    """Above 64 rows: dequantise into the scratch, then the unchanged bf16 GEMM (its tolerance)."""
    N, K = 1024, 512
    g = torch.Generator(device=gpu).manual_seed(M)
    codes, e = ref.mx4_quantize((0.02 * torch.randn(N, K, generator=g, device=gpu)).to(torch.bfloat16))
    x = torch.randn(M, K, generator=g, device=gpu).to(torch.bfloat16)
    out = ops.gemm_mx4(x, ops.mx4_pack(codes, e), epi=epi)
    exp = x.float() @ ref.mx4_dequant(codes, e).float().T
    if epi:
        exp = ref.silu_mul(ops.deinterleave_cols(exp.to(torch.bfloat16))).float()
    torch.testing.assert_close(out.float(), exp, atol=2e-2 * exp.abs().max().item() / 4 + 1e-2, rtol=2e-2)
