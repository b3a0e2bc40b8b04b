#!/usr/bin/env python
"""Dump the GEMM planner's query ops over the projection shapes of the preset models, to compare
two builds on one GPU (a planner refactor must leave every answer as it was).

Uses only ops that predate the gemm_plan.cc planner: gemm_workspace, gemm_sk_workgroups,
gemm_rope_supported, w4_chain_ok, mid_chain_ok (with gemm_mid_chain 0 and 1) and
gemv_chain_supported.  For every (N, K) of qkv / o / gate_up / down / lm_head of the non-tiny
presets at TP 1, 2, 4, 8 and every M in 1..8192, 12288, 16384, one line per maximal M interval
with constant answers; the sha256 of the whole dump is printed last.

    python scripts/dump_gemm_predicates.py [out.txt]
"""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from mlopamd import ops  # noqa: E402
from mlopamd.models.config import PRESETS  # noqa: E402


def nk_shapes():
    out = set()
    for cfg in PRESETS.values():
        if cfg.name.startswith("tiny"):
            continue
        H, I, D = cfg.hidden_size, cfg.intermediate_size, cfg.head_dim
        for tp in (1, 2, 4, 8):
            hq, hkv = cfg.num_heads // tp, max(cfg.num_kv_heads // tp, 1)
            out |= {((hq + 2 * hkv) * D, H), (H, hq * D), (2 * I // tp, H), (H, I // tp), (cfg.vocab_size // tp, H)}
    return sorted(out)


def main():
    ops.load()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    ops._sk_reserve(dev)
    o = torch.ops.mlop
    ms = list(range(1, 8193)) + [12288, 16384]
    lines = []
    for N, K in nk_shapes():
        cur, first, last = None, 0, 0
        for M in ms:
            v = [o.gemm_workspace(M, N, K, 0) // (M * N), o.gemm_workspace(M, N, K, 1) // (M * N),
                 o.gemm_workspace(M, N, K, 2) // (M * N), o.gemm_sk_workgroups(M, N, K),
                 int(o.gemm_rope_supported(M, N, K)), int(o.w4_chain_ok(M, N, K))]
            v += [int(o.gemv_chain_supported(M, N, K, e)) for e in (0, 1, 3)]
            if M <= 64:  # mid_chain_ok is false above 64 rows whatever the switch says
                for mode in (0, 1):
                    o.gemm_mid_chain(mode)
                    v += [int(o.mid_chain_ok(M, N, K, e)) for e in (0, 1, 3)]
                o.gemm_mid_chain(0)
            if v != cur:
                if cur is not None:
                    lines.append(f"{N} {K} | {first} {last} | {' '.join(map(str, cur))}")
                cur, first = v, M
            last = M
        lines.append(f"{N} {K} | {first} {last} | {' '.join(map(str, cur))}")
    text = "\n".join(lines) + "\n"
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(text)
    print(f"{len(lines)} lines, sha256 {hashlib.sha256(text.encode()).hexdigest()}")


if __name__ == "__main__":
    main()
