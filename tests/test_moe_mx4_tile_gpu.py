"""moe_mx4t.hip on the GPU against ops/reference.py, in test_moe_mx4_kernels_gpu's shape: an exact one-hot probe, fp64
with gemm_mx4's derived bound, the fused SiLU-mul, graph replays under changing routing, ops.grouped_gemm_mx4's routing."""
import pytest
import torch

from mlopamd import ops
from mlopamd.ops import reference as ref
from test_moe_mx4_kernels_gpu import _experts, _offsets, _ulp

pytestmark = pytest.mark.gpu
COUNTS = [0, 130, 1, 17, 128]  # an empty expert, two M-tiles (2 rows in the second), 1 row, a ragged row tile, a full tile
LIVE8 = {3: 1, 17: 2, 31: 3, 64: 1, 65: 2, 100: 3, 126: 1, 127: 2}
CASES = [(5, 256, 640, COUNTS),                                            # 5 K tiles: prologue and tail only
         (4, 128, 1792, [33, 64, 65, 0]),                                  # 14 K tiles: the steady loop
         (128, 128, 128, [LIVE8.get(i, 0) for i in range(128)])]           # the scan past 64 experts, early exits


def _run(x, W, off, R, epi=ops.EPI_NONE, a_rows=None):
    """R permuted rows into a sentinel-filled buffer with three rows to spare, which must stay untouched."""
    out = torch.full((R + 3, W.N if epi == ops.EPI_NONE else W.N // 2), 7.0, device=x.device, dtype=torch.bfloat16)
    torch.ops.mlop.grouped_gemm_mx4_tile(out[:R], x, W.qw, W.qe, off, W.N, epi, a_rows)
    assert bool((out[R:] == 7.0).all())
    return out[:R]


@pytest.mark.parametrize("mapped", [False, True], ids=["gathered", "a_rows"])
@pytest.mark.parametrize("c", range(8))
def test_exact_probe(gpu, c, mapped):
    """x[r, (8 r + c) % K] = 1: output row r is that column of its expert's dequantised weight, exactly."""
    E, N, K, R = 5, 256, 512, sum(COUNTS)
    codes, e = _experts(E, N, K, gpu, c, 2, 252)
    e.view(-1)[:4] = torch.tensor([2, 3, 251, 252], dtype=torch.uint8, device=gpu)
    rows = torch.arange(R, device=gpu)
    cols = (8 * rows + c) % K
    x = torch.zeros(R, K, device=gpu, dtype=torch.bfloat16)
    x[rows, cols] = 1
    a_rows = None
    if mapped:  # permuted row r is row a_rows[r] of the token matrix
        a_rows = torch.randperm(R, generator=torch.Generator().manual_seed(c)).to(gpu, torch.int32)
        xs = torch.empty_like(x)
        xs[a_rows.long()] = x
        x = xs
    expert = torch.repeat_interleave(torch.arange(E, device=gpu), torch.tensor(COUNTS, device=gpu))
    want = ref.mx4_dequant(codes.view(E * N, K), e.view(E * N, -1)).view(E, N, K)[expert, :, cols]
    assert torch.equal(_run(x, ops.mx4_experts_pack(codes, e), _offsets(COUNTS, gpu), R, a_rows=a_rows), want)


@pytest.fixture(scope="module")
def fp64_cases(gpu):
    """Per case: packed experts, offsets, activations, the fp64 product and the magnitude sum, computed once."""
    made = []
    for i, (E, N, K, counts) in enumerate(CASES):
        codes, e = _experts(E, N, K, gpu, 11 + i, 120, 130)
        x = torch.randn(sum(counts), K, device=gpu, dtype=torch.bfloat16, generator=torch.Generator(device=gpu).manual_seed(i))
        deq = ref.mx4_dequant(codes.view(E * N, K), e.view(E * N, -1)).view(E, N, K).double()
        expert = torch.repeat_interleave(torch.arange(E, device=gpu), torch.tensor(counts, device=gpu))
        exp = torch.einsum("rk,rnk->rn", x.double(), deq[expert])
        mag = torch.einsum("rk,rnk->rn", x.double().abs(), deq[expert].abs())
        made.append((ops.mx4_experts_pack(codes, e), _offsets(counts, gpu), x, exp, mag))
    return made


@pytest.mark.parametrize("i", range(3), ids=[f"E{c[0]}-N{c[1]}-K{c[2]}" for c in CASES])
def test_tile_vs_fp64_and_fused_silu_mul(gpu, fp64_cases, i):
    """Plain: |out - ref| <= 2^-8 |ref| + K 2^-24 sum_k |w x| (test_gemm_mx4_vs_fp64's bound), a relaunch bit-identical.
    SiLU-mul over the plain launch's bf16 gate and up (test_moe_mx4_kernels_gpu's): |out - ref| <= |u| ulp(silu) + ulp(ref)."""
    W, off, x, exp, mag = fp64_cases[i]
    out = _run(x, W, off, x.shape[0])
    assert torch.equal(_run(x, W, off, x.shape[0]), out)
    assert bool(((out.double() - exp).abs() <= 2.0 ** -8 * exp.abs() + W.K * 2.0 ** -24 * mag).all())
    y = ops.deinterleave_cols(out)
    s, u, want = torch.nn.functional.silu(y[:, : W.N // 2].float()).to(y.dtype).float(), y[:, W.N // 2:].float(), ref.silu_mul(y).float()
    out = _run(x, W, off, x.shape[0], ops.EPI_SILU_MUL)
    assert bool(((out.float() - want).abs() <= u.abs() * _ulp(s) + _ulp(want)).all())


def test_graph_replays_follow_the_routing(gpu, fp64_cases):
    """One captured launch over an offsets buffer: each replay, after other counts of the same total (one with
    empty experts) were copied into it, equals the eager launch on those counts."""
    W, _off, x, _exp, _mag = fp64_cases[0]
    routings = [COUNTS, [276, 0, 0, 0, 0], [64, 65, 16, 1, 130]]
    eager = [_run(x, W, _offsets(c, gpu), 276) for c in routings]
    off, out, graph = _offsets(COUNTS, gpu), torch.empty(276, W.N, device=gpu, dtype=torch.bfloat16), torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        torch.ops.mlop.grouped_gemm_mx4_tile(out, x, W.qw, W.qe, off, W.N, ops.EPI_NONE, None)
    for i in (1, 2, 0):
        off.copy_(_offsets(routings[i], gpu))
        graph.replay()
        assert torch.equal(out, eager[i]), i


def test_routing(gpu, fp64_cases, monkeypatch):
    """The tile kernel inside (MIN, MAX] at N % 128 == 0; every other call where it went: the streaming kernel (at MIN, MAX = 0,
    N = 48) or dequantise + grouped_gemm (N = 96 above MX4_MOE_MAX_AVG_ROWS: grouped_gemm itself needs N % 32 == 0)."""
    W, off, x, _exp, _mag = fp64_cases[0]

    def stream(W):
        out = torch.empty(x.shape[0], W.N, device=gpu, dtype=torch.bfloat16)
        torch.ops.mlop.grouped_gemm_mx4(out, x, W.qw, W.qe, off, W.N, ops.EPI_NONE, 0, None)
        return out

    for knob, v in (("TILE_MIN_AVG_ROWS", 64), ("TILE_MAX_AVG_ROWS", 512), ("MAX_AVG_ROWS", 256)):
        monkeypatch.setattr(ops, "MX4_MOE_" + knob, v)
    tile = _run(x, W, off, x.shape[0])
    assert torch.equal(ops.grouped_gemm_mx4(x, W, off, avg_rows=65), tile)
    assert torch.equal(ops.grouped_gemm_mx4(x, W, off, avg_rows=512), tile)
    assert torch.equal(ops.grouped_gemm_mx4(x, W, off, avg_rows=64), stream(W))
    for N in (48, 96):
        Wn = ops.mx4_experts_pack(*_experts(5, N, 640, gpu, N, 120, 130))
        assert torch.equal(ops.grouped_gemm_mx4(x, Wn, off, avg_rows=200), stream(Wn)), N
    want = ops.grouped_gemm(x, ops.mx4_experts_dequant(Wn), off, avg_rows=300)
    assert torch.equal(ops.grouped_gemm_mx4(x, Wn, off, avg_rows=300), want)
    monkeypatch.setattr(ops, "MX4_MOE_TILE_MAX_AVG_ROWS", 0)
    assert torch.equal(ops.grouped_gemm_mx4(x, W, off, avg_rows=200), stream(W))
