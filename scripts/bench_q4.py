"""Int4 weights (gemm_q4.hip) against the bf16 route, on one GPU, A and B alternating in one process.

    python scripts/bench_q4.py kernel          # the projections: us, achieved TB/s of packed bytes
    python scripts/bench_q4.py engine          # a Llama-3-8B engine with bf16 and with int4 weights

kernel: the four Llama-3-8B projections and 70B's gate_up.  M <= 64: ``ops.gemm_q4`` (the int4 kernel)
against ``ops.gemm`` over the bf16 weight; M = 128, 512, 2048: dequantise + GEMM against the GEMM alone.
Each timed window flushes nothing: like the decode loop, every call streams weights that the other
projections' traffic has pushed out of the caches (the weights rotate over enough copies to exceed them).
Device events; one JSON line per (shape, M) with the median of the rounds and their min / max.
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

from mlopamd import ops  # noqa: E402
from mlopamd.models import build_model  # noqa: E402
from mlopamd.models.config import get_config  # noqa: E402
from mlopamd.runtime.engine import Engine, EngineConfig  # noqa: E402
from mlopamd.runtime.sampler import SamplingParams  # noqa: E402

SHAPES = {"8b-qkv": (6144, 4096), "8b-o": (4096, 4096), "8b-gate_up": (28672, 4096), "8b-down": (4096, 14336),
          "70b-gate_up": (57344, 8192)}
CACHE_BYTES = 512 * 2 ** 20  # rotate over more weight bytes than L2 + MALL hold


def _time(fn, n_copies, iters, rounds):
    """us per call: ``rounds`` windows of ``iters`` calls, fn(i) using weight copy i % n_copies."""
    out = []
    for i in range(2 * n_copies):
        fn(i)
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for i in range(iters):
            fn(i)
        b.record()
        b.synchronize()
        out.append(1e3 * a.elapsed_time(b) / iters)
    return out


def bench_kernel(args):
    dev = torch.device("cuda", 0)
    ops.load()
    for name, (N, K) in SHAPES.items():
        if args.shapes and name not in args.shapes:
            continue
        copies = max(2, -(-CACHE_BYTES // ops.q4_bytes(N, K)))
        copies = min(copies, max(2, int(8 * 2 ** 30 // (2 * N * K))))  # bf16 copies: at most 8 GiB
        wb = [(0.02 * torch.randn(N, K, device=dev)).to(torch.bfloat16) for _ in range(copies)]
        wq = [ops.q4_quantize_pack(w) for w in wb]
        ops.q4_reserve_scratch(dev, N * K)
        for M in args.rows:
            x = torch.randn(M, K, device=dev, dtype=torch.bfloat16)
            iters = max(8, min(200, int(2e9 // (N * K * max(M, 16) // 16))))
            fa = lambda i: ops.gemm(x, wb[i % copies])  # noqa: E731
            fb = lambda i: ops.gemm_q4(x, wq[i % copies])  # noqa: E731
            ta, tb = [], []
            for _ in range(args.rounds):  # A, B, A, B ...
                ta += _time(fa, copies, iters, 1)
                tb += _time(fb, copies, iters, 1)
            ma, mb = statistics.median(ta), statistics.median(tb)
            row = dict(bench="kernel", shape=name, N=N, K=K, M=M, route="int4-kernel" if M <= ops.Q4_WS_MAX_M else "dequant+gemm",
                       bf16_us=round(ma, 2), bf16_min=round(min(ta), 2), bf16_max=round(max(ta), 2),
                       int4_us=round(mb, 2), int4_min=round(min(tb), 2), int4_max=round(max(tb), 2),
                       speedup=round(ma / mb, 3), bf16_TBps=round(2 * N * K / ma / 1e6, 3),
                       int4_TBps=round(ops.q4_bytes(N, K) / mb / 1e6, 3))
            print(json.dumps(row), flush=True)
        del wb, wq
        torch.cuda.empty_cache()


def bench_engine(args):
    dev = torch.device("cuda", 0)
    ops.load()
    cfg = get_config("llama3-8b", num_layers=args.layers)
    g = torch.Generator().manual_seed(0)
    for rnd in range(args.rounds):
        for wd in ("bf16", "int4"):
            model = build_model(cfg, device=dev, seed=0)
            eng = Engine(model, EngineConfig(max_num_seqs=64, max_num_batched_tokens=2048, max_model_len=4096,
                                             num_kv_blocks=2048, graph_buckets=(1, 8, 64), weight_dtype=wd))
            row = dict(bench="engine", round=rnd, weight_dtype=wd, layers=cfg.num_layers,
                       weight_gb=round(model.weight_bytes() / 1e9, 3))
            for batch in (1, 8, 64):
                prompts = [torch.randint(2, 1000, (16,), generator=g).tolist() for _ in range(batch)]
                sp = SamplingParams(max_tokens=args.gen, ignore_eos=True)
                eng.generate(prompts, SamplingParams(max_tokens=8, ignore_eos=True))  # warm-up, graph capture
                torch.cuda.synchronize()
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                eng.generate(prompts, sp)
                b.record()
                b.synchronize()
                row[f"decode_tok_s_b{batch}"] = round(batch * args.gen / (a.elapsed_time(b) / 1e3), 1)
            prompts = [torch.randint(2, 1000, (2048,), generator=g).tolist() for _ in range(4)]
            eng.generate(prompts[:1], SamplingParams(max_tokens=1, ignore_eos=True))
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            eng.generate(prompts, SamplingParams(max_tokens=1, ignore_eos=True))
            b.record()
            b.synchronize()
            row["prefill_tok_s"] = round(4 * 2048 / (a.elapsed_time(b) / 1e3), 1)
            print(json.dumps(row), flush=True)
            del eng, model
            torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("what", choices=["kernel", "engine"])
    ap.add_argument("--rows", type=int, nargs="*", default=[1, 4, 8, 16, 32, 64, 128, 512, 2048])
    ap.add_argument("--shapes", nargs="*", default=[])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--gen", type=int, default=128)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_q4 measures on a GPU"
    (bench_kernel if args.what == "kernel" else bench_engine)(args)


if __name__ == "__main__":
    main()
