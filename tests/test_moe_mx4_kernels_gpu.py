"""moe_mx4.hip on the GPU against ops/reference.py: an exact one-hot probe (empty expert, the
64-row chunk loop, a ragged last tile, gathered rows and a row map, every row-block count), fp64
with gemm_mx4's derived bound, the fused SiLU-mul against the unfused path, and the dequantise +
grouped_gemm route.  Scale bytes as in test_mx4_kernels_gpu: [2, 252] where the test is exact."""
import pytest
import torch

from mlopamd import ops
from mlopamd.ops import reference as ref

pytestmark = pytest.mark.gpu
LIVE8 = {3: 1, 17: 2, 31: 3, 64: 1, 65: 2, 100: 3, 126: 1, 127: 2}
CASES = [(4, 32, 128, [1, 0, 5, 16]),                                      # one K tile: three waves idle
         (4, 512, 256, [33, 64, 65, 0]),                                   # TINY_MIXTRAL's w13
         (128, 256, 256, [LIVE8.get(i, 0) for i in range(128)]),           # 8 live experts, 120 empty
         (8, 48, 640, [130, 0, 0, 0, 0, 0, 0, 2])]                         # uneven wave split, RB = 1, three chunks
# SiLU-mul pairs a block of 16 gate rows with the next 16 up rows (ops.interleave_gate_up): N % 32 == 0,
# which N = 48 is not, so that case has no SiLU-mul form
EPI_CASES = [(c, epi) for c in CASES for epi in (ops.EPI_NONE, ops.EPI_SILU_MUL) if epi == ops.EPI_NONE or c[1] % 32 == 0]


def _experts(E, N, K, dev, seed, e_lo, e_hi):
    g = torch.Generator(device=dev).manual_seed(seed)
    codes = torch.randint(0, 16, (E, N, K), generator=g, device=dev, dtype=torch.uint8)
    e = torch.randint(e_lo, e_hi + 1, (E, N, K // 32), generator=g, device=dev, dtype=torch.uint8)
    return codes, e


def _offsets(counts, dev):
    return torch.tensor([0, *torch.tensor(counts).cumsum(0).tolist()], dtype=torch.int32, device=dev)


def _run(x, W, off, R, epi=ops.EPI_NONE, rb=0, a_rows=None):
    """R permuted rows into a sentinel-filled buffer with three rows to spare."""
    out = torch.full((R + 3, W.N if epi == ops.EPI_NONE else W.N // 2), 7.0, device=x.device, dtype=torch.bfloat16)
    torch.ops.mlop.grouped_gemm_mx4(out[:R], x, W.qw, W.qe, off, W.N, epi, rb, a_rows)
    return out


@pytest.mark.parametrize("mapped", [False, True], ids=["gathered", "a_rows"])
@pytest.mark.parametrize("c", range(8))
def test_exact_probe(gpu, c, mapped):
    """x[r, 8 (r % 64) + c] = 1: output row r is column 8 (r % 64) + c of its expert's dequantised
    weight, exactly, for every k, wave, code and scale byte; rows behind offsets[-1] stay untouched."""
    E, N, K, counts, R = 4, 64, 512, [0, 70, 1, 17], 96
    codes, e = _experts(E, N, K, gpu, c, 2, 252)
    e.view(-1)[:4] = torch.tensor([2, 3, 251, 252], dtype=torch.uint8, device=gpu)
    W, off, n = ops.mx4_experts_pack(codes, e), _offsets(counts, gpu), sum(counts)
    rows = torch.arange(R, device=gpu)
    cols = 8 * (rows % 64) + c
    x = torch.zeros(R, K, device=gpu, dtype=torch.bfloat16)
    x[rows, cols] = 1
    a_rows = None
    if mapped:  # permuted row r is row a_rows[r] of the token matrix
        a_rows = torch.randperm(R, generator=torch.Generator().manual_seed(c)).to(gpu, torch.int32)
        xs = torch.empty_like(x)
        xs[a_rows.long()] = x
        x = xs
    expert = torch.repeat_interleave(torch.arange(E, device=gpu), torch.tensor(counts, device=gpu))
    want = ref.mx4_dequant(codes.view(E * N, K), e.view(E * N, -1)).view(E, N, K)[expert, :, cols[:n]]
    assert torch.equal(ops.grouped_gemm_mx4(x, W, off, a_rows=a_rows)[:n], want)
    for rb in (1, 2, 4):
        out = _run(x, W, off, R, rb=rb, a_rows=a_rows)
        assert torch.equal(out[:n], want), rb
        assert bool((out[n:] == 7.0).all()), rb


@pytest.fixture(scope="module")
def fp64_cases(gpu):
    """Per case: packed experts, offsets, activations, the fp64 product and the magnitude sum, computed once."""
    made = {}
    for i, (E, N, K, counts) in enumerate(CASES):
        codes, e = _experts(E, N, K, gpu, 11 + i, 120, 130)
        R = sum(counts)
        x = torch.randn(R, K, device=gpu, dtype=torch.bfloat16, generator=torch.Generator(device=gpu).manual_seed(i))
        deq = ref.mx4_dequant(codes.view(E * N, K), e.view(E * N, -1)).view(E, N, K).double()
        expert = torch.repeat_interleave(torch.arange(E, device=gpu), torch.tensor(counts, device=gpu))
        exp = torch.einsum("rk,rnk->rn", x.double(), deq[expert])
        mag = torch.einsum("rk,rnk->rn", x.double().abs(), deq[expert].abs())
        made[(E, N, K)] = (ops.mx4_experts_pack(codes, e), _offsets(counts, gpu), x, exp, mag)
    return made


@pytest.mark.parametrize("case,epi", EPI_CASES, ids=[f"E{c[0]}-N{c[1]}-K{c[2]}-epi{epi}" for c, epi in EPI_CASES])
def test_grouped_gemm_mx4_vs_fp64(gpu, fp64_cases, case, epi):
    """Rows behind the last expert keep their sentinel; a relaunch is bit-identical.  Plain:
    |out - ref| <= 2^-8 |ref| + K 2^-24 sum_k |w x| (test_gemm_mx4_vs_fp64's bound).  SiLU-mul: within
    one bf16 ulp of ref.silu_mul of the bf16-rounded fp64 product."""
    E, N, K, counts = case
    W, off, x, exp, mag = fp64_cases[(E, N, K)]
    R = sum(counts)
    out = _run(x, W, off, R, epi)
    assert bool((out[R:] == 7.0).all())
    assert torch.equal(_run(x, W, off, R, epi), out)
    if epi == ops.EPI_NONE:
        err, bound = (out[:R].double() - exp).abs(), 2.0 ** -8 * exp.abs() + K * 2.0 ** -24 * mag
    else:
        want = ref.silu_mul(ops.deinterleave_cols(exp.to(torch.bfloat16))).double()
        err, bound = (out[:R].double() - want).abs(), _ulp(want)
    print(f"worst error / bound {float((err / bound.clamp_min(1e-300)).max()):.3f}, "
          f"{int((err > bound).sum())} of {err.numel()} above it")
    assert bool((err <= bound).all())


def _ulp(v):
    return torch.ldexp(torch.ones_like(v), torch.frexp(v)[1] - 8)


@pytest.mark.parametrize("case", [c for c in CASES if c[1] % 32 == 0], ids=lambda c: f"E{c[0]}-N{c[1]}")
def test_silu_mul_epilogue_rounds_as_the_plain_launch(gpu, fp64_cases, case):
    """The fused epilogue rounds both sums to bf16 as the plain launch stores them, then is
    ref.silu_mul of those.  __expf and v_rcp_f32 are within 2^-17 of fp32's exp and division, so the
    kernel's bf16 silu is the reference's or its neighbour: |out - ref| <= |u| ulp(silu) + ulp(ref).
    Both row-block counts it can run with give the same bits."""
    E, N, K, counts = case
    W, off, x, _exp, _mag = fp64_cases[(E, N, K)]
    R = sum(counts)
    y = ops.deinterleave_cols(_run(x, W, off, R)[:R])
    s, u, want = torch.nn.functional.silu(y[:, : N // 2].float()).to(y.dtype).float(), y[:, N // 2:].float(), ref.silu_mul(y).float()
    out = _run(x, W, off, R, ops.EPI_SILU_MUL, 2)[:R]
    assert bool(((out.float() - want).abs() <= u.abs() * _ulp(s) + _ulp(want)).all())
    if N % 64 == 0:
        assert torch.equal(_run(x, W, off, R, ops.EPI_SILU_MUL, 4)[:R], out)


@pytest.mark.parametrize("epi", [ops.EPI_NONE, ops.EPI_SILU_MUL])
def test_large_route(gpu, epi):
    """avg_rows above MX4_MOE_MAX_AVG_ROWS: dequantise the experts, then the unchanged grouped GEMM
    (test_gemm_mx4_large_m_route's tolerance)."""
    E, N, K, counts = 4, 512, 256, [70, 66, 80, 64]
    g = torch.Generator(device=gpu).manual_seed(5)
    w = (0.02 * torch.randn(E, N, K, generator=g, device=gpu)).to(torch.bfloat16)
    W = ops.mx4_experts_quantize_pack(w)
    x = torch.randn(sum(counts), K, generator=g, device=gpu).to(torch.bfloat16)
    out = ops.grouped_gemm_mx4(x, W, _offsets(counts, gpu), epi=epi, avg_rows=ops.MX4_MOE_MAX_AVG_ROWS + 1)
    expert = torch.repeat_interleave(torch.arange(E, device=gpu), torch.tensor(counts, device=gpu))
    codes, e = ops.mx4_experts_unpack(W)
    deq = ref.mx4_dequant(codes.view(E * N, K), e.view(E * N, -1)).view(E, N, K)
    exp = torch.einsum("rk,rnk->rn", x.float(), deq.float()[expert])
    if epi:
        exp = ref.silu_mul(ops.deinterleave_cols(exp.to(torch.bfloat16))).float()
    torch.testing.assert_close(out.float(), exp, atol=2e-2 * exp.abs().max().item() / 4 + 1e-2, rtol=2e-2)
