"""The sampler (K10) with and without its extensions at the headline's shapes: n = 256 and
n = 2048 rows x V = 128256 bf16 logits.  Three cases per population (greedy rows; temperature
0.8 / top-k 50 / top-p 0.9 rows): plain, every row penalised, every row penalised with
logprobs = 5.  Microseconds per ``Sampler`` call (device events, warmed, >= 200 calls), then the
extended path's stages on their own (fp32 copy, apply_penalties, the draw, penalty_update,
token_logprobs) and the bytes a penalised row moves over apply_penalties' time.  One JSON line
per measurement; results: profiles/sampler_penalties_logprobs.md."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mlopamd import ops  # noqa: E402
from mlopamd.runtime.sampler import Sampler, SamplerExt, SamplingParams  # noqa: E402

ap = argparse.ArgumentParser(description=__doc__)
ap.add_argument("--rows", type=int, nargs="+", default=[256, 2048])
ap.add_argument("--vocab", type=int, default=128256)
ap.add_argument("--calls", type=int, default=200)
ap.add_argument("--prompt", type=int, default=512, help="prompt ids per penalised row's table slot")
ap.add_argument("--generated", type=int, default=128, help="output ids counted per slot")
args = ap.parse_args()

ops.load()
dev = torch.device("cuda")
V = args.vocab


def timeit(fn, calls):
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(calls):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / calls * 1e3


def emit(**kw):
    print(json.dumps(kw), flush=True)


for n in args.rows:
    torch.manual_seed(0)
    logits = (3 * torch.randn(n, V, device=dev)).to(torch.bfloat16)
    table = ops.penalty_table(n, V, dev)
    rng = np.random.default_rng(0)
    for s in range(n):
        ops.penalty_reset(table, s, rng.integers(0, V, size=args.prompt), rng.integers(0, V, size=args.generated), V)
    snapshot = table.clone()
    touched16 = int((table.view(n, -1, 4) != 0).any(-1).sum()) // n  # 16-B logits chunks rewritten per row
    sampler = Sampler(dev)
    gi = np.zeros(n, np.int64)
    slots, none = np.arange(n, dtype=np.int32), np.full(n, -1, np.int32)
    for pop, base in (("greedy", {}), ("random", dict(temperature=0.8, top_k=50, top_p=0.9))):
        plain = [SamplingParams(**base)] * n
        pen = [SamplingParams(repetition_penalty=1.3, frequency_penalty=0.5, presence_penalty=0.4, **base)] * n
        rep, freq, pres = np.full(n, 1.3, np.float32), np.full(n, 0.5, np.float32), np.full(n, 0.4, np.float32)
        ext_pen = SamplerExt(table, slots, rep, freq, pres, none, V)
        ext_lp = SamplerExt(table, slots, rep, freq, pres, np.full(n, 5, np.int32), V)
        t_plain = timeit(lambda: sampler(logits, plain, gi), args.calls)
        t_pen = timeit(lambda: sampler.sample_ext(logits, pen, ext_pen, gi), args.calls)
        table.copy_(snapshot)  # the timed draws were counted: back to the same table for the next case
        t_lp = timeit(lambda: sampler.sample_ext(logits, pen, ext_lp, gi), args.calls)
        table.copy_(snapshot)
        emit(n=n, V=V, rows=pop, plain_us=round(t_plain, 1), penalised_us=round(t_pen, 1),
             penalised_logprobs5_us=round(t_lp, 1), penalised_over_plain=round(t_pen / t_plain, 2),
             penalised_logprobs5_over_plain=round(t_lp / t_plain, 2))
    # the extended path's stages on their own
    d = {k: torch.from_numpy(a).to(dev) for k, a in (("slots", slots), ("rep", rep), ("freq", freq), ("pres", pres))}
    work = logits.float()
    toks = ops.argmax(logits)
    want = torch.full((n,), 5, dtype=torch.int32, device=dev)
    lp = torch.zeros(n, 6, device=dev)
    ids = torch.zeros(n, 6, dtype=torch.int32, device=dev)
    temps = torch.full((n,), 0.8, device=dev)
    ks = torch.full((n,), 50, dtype=torch.int32, device=dev)
    ps = torch.full((n,), 0.9, device=dev)
    u = torch.rand(n, device=dev)
    t_copy = timeit(lambda: logits.float(), args.calls)
    t_apply = timeit(lambda: ops.apply_penalties(work, table, d["slots"], d["rep"], d["freq"], d["pres"]), args.calls)
    t_amax = timeit(lambda: ops.argmax(work), args.calls)
    t_amax_bf = timeit(lambda: ops.argmax(logits), args.calls)
    t_draw = timeit(lambda: ops.sample(work, temps, ks, ps, u, full=False), args.calls)
    t_upd = timeit(lambda: ops.penalty_update(table, d["slots"], toks, V), args.calls)
    t_lps = timeit(lambda: ops.token_logprobs(lp, ids, logits, toks, want), args.calls)
    row_bytes = 4 * table.shape[1] + 2 * 16 * touched16  # the table row, + the touched logits read and written
    emit(n=n, V=V, stage_us=dict(fp32_copy=round(t_copy, 1), apply_penalties=round(t_apply, 1),
                                 argmax_f32=round(t_amax, 1), argmax_bf16=round(t_amax_bf, 1),
                                 sample_topk50=round(t_draw, 1), penalty_update=round(t_upd, 1),
                                 token_logprobs5_bf16=round(t_lps, 1)),
         penalised_row_bytes=row_bytes, touched_16B_chunks_per_row=touched16,
         apply_penalties_TBps=round(n * row_bytes / t_apply / 1e6, 2),
         fp32_copy_TBps=round(n * V * 6 / t_copy / 1e6, 2),
         token_logprobs_TBps=round(n * V * 2 / t_lps / 1e6, 2))
    del logits, table, snapshot, work
    torch.cuda.empty_cache()
