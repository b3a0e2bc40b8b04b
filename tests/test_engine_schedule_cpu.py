"""The engine's schedule on the CPU, pinned: every launch and every step of one workload.

One workload (14 prompts of 3-49 tokens, every third behind a shared 32-token prefix, one request
added every second iteration, the newest aborted at iteration 12, 9 KV pages so that sequences
are preempted) runs on a CPU TINY_LLAMA engine in each configuration of ``RUNS``: one-step-ahead,
synchronous mixed and ``mixed_prefill=False`` scheduling, ``prefill_min_batch`` 1 and 2, a
sliding-window model that releases pages, two LoRA adapters, and decode "graphs" (stand-ins whose
``replay()`` runs the eager forward over the padded metadata, so the bucketed branch of the step
builder runs without a GPU).  The trace has one line per ``step()``,

    S <tracer kind> <seq id>[*] ... | <seq id>=<finish reason> ...        (*: finished)

followed on the same line, to keep the fixture short, by one record per ``Engine._launch`` of that
step (the method is wrapped):

    || L kind T nt nl part nparts bucket npt=<flash tiles> g=<greedy> ids=<B of the device-side
       id gather, or -> lora=<0/1> meta=<crc32 of the metadata words the upload ships, token ids
       zeroed> [ts=<crc32 of the per-token adapter slots>]

and at the end every ``stats`` entry that is not a time.  All requests ignore EOS and
have no stop tokens, so nothing depends on a sampled token's value and the trace is the same for
every model seed and on every CPU (a test checks two seeds).

The traces are compared byte for byte with tests/fixtures/engine_schedule.txt, so a change of what
the engine schedules or launches shows up as a diff of that file.  The fixture was recorded before
the step builders were unified and pins that behaviour; regenerate it with
``python tests/test_engine_schedule_cpu.py --write`` only for a change that is MEANT to alter the
schedule, and review the diff.
"""
import dataclasses
import os
import sys
import zlib

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
FIXTURE = os.path.join(ROOT, "tests", "fixtures", "engine_schedule.txt")

from mlopamd.models import build_model  # noqa: E402
from mlopamd.models.config import TINY_LLAMA  # noqa: E402
from mlopamd.runtime.attn_meta import plan_partitions  # noqa: E402
from mlopamd.runtime.engine import Engine, EngineConfig  # noqa: E402
from mlopamd.runtime.sampler import SamplingParams  # noqa: E402

BASE = dict(max_num_seqs=5, max_num_batched_tokens=40, max_model_len=256, num_kv_blocks=9, mixed_min_chunk=8,
            prefill_min_batch=2, max_decode_gap=3, use_graphs=False)
ASYNC, SYNC, SPLIT = {}, {"async_scheduling": False}, {"async_scheduling": False, "mixed_prefill": False}
# name -> (engine configuration over BASE, sliding window, adapters, stand-in graphs)
RUNS = {
    "async": (ASYNC, 0, False, False),
    "sync_mixed": (SYNC, 0, False, False),
    "sync_split": (SPLIT, 0, False, False),
    "async_pmb1": ({**ASYNC, "prefill_min_batch": 1}, 0, False, False),
    "sync_mixed_pmb1": ({**SYNC, "prefill_min_batch": 1}, 0, False, False),
    "async_swa16": (ASYNC, 16, False, False),
    "async_lora": ({**ASYNC, "max_adapters": 2, "max_lora_rank": 8}, 0, True, False),
    "sync_mixed_lora": ({**SYNC, "max_adapters": 2, "max_lora_rank": 8}, 0, True, False),
    "async_graphs": (ASYNC, 0, False, True),
    "sync_mixed_graphs": (SYNC, 0, False, True),
}


def workload():
    rng = np.random.default_rng(11)
    shared = rng.integers(2, 500, size=32).tolist()
    prompts = [rng.integers(2, 500, size=int(rng.integers(3, 50))).tolist() for _ in range(14)]
    return [shared + p if i % 3 == 2 else p for i, p in enumerate(prompts)]


class _StandInGraph:
    """What ``Engine.graphs[bucket]`` holds, without a GPU: ``replay()`` runs the eager forward of
    the bucket's padded rows into the fixed logits buffer, as a captured decode graph would."""

    def __init__(self, eng, b):
        m = eng.model
        self.eng, self.b = eng, b
        self.part = plan_partitions(b, m.n_kv, eng.meta.span(eng.max_model_len))
        self.logits = torch.zeros(b, m.cfg.vocab_size, dtype=torch.float32)

    def replay(self):
        eng, b = self.eng, self.b
        meta = eng.meta.meta(b, b, b, *self.part)
        self.logits.copy_(eng.model.logits_local(eng.model.forward(eng.meta.ids_d[:b], meta, eng.kv)))


def _crc(a) -> str:
    return "%08x" % zlib.crc32(np.ascontiguousarray(a).tobytes())


def trace(name, seed=1, adapter_dirs=None):
    kw, window, lora, graphs = RUNS[name]
    cfg = dataclasses.replace(TINY_LLAMA, sliding_window=window) if window else TINY_LLAMA
    model = build_model(cfg, device="cpu", dtype=torch.float32, seed=seed)
    eng = Engine(model, EngineConfig(**{**BASE, **kw}))
    names = [None] * 14
    if lora:
        eng.load_adapter("x", adapter_dirs["x"])
        eng.load_adapter("y", adapter_dirs["y"])
        names = [("x", "y", None)[i % 3] for i in range(14)]
    if graphs:
        for b in (1, 2, 4, 8):
            if b in eng.buckets:
                g = _StandInGraph(eng, b)
                eng.graphs[b] = (g, g.logits)
    lines, launched = [f"# run {name}"], []
    real_launch = eng._launch
    meta = eng.meta

    def launch(kind, T, nt, nl, part, nparts, bucket, greedy=False):
        words = meta.hn[:meta.extent(eng.rows_hi)].copy()
        ids = meta.ids_h.storage_offset() * 2  # the ids region (int64) in int32 words
        words[ids:ids + 2 * meta.max_tokens] = 0
        g = eng._ids_gather
        line = (f"L {kind} {T} {nt} {nl} {part} {nparts} {bucket} npt={meta.npt} g={int(bool(greedy))} "
                f"ids={'-' if g is None else g[0]} lora={int(eng._step_lora)} meta={_crc(words)}")
        if eng.lora is not None:
            line += f" ts={_crc(eng._ts_hn[:T])}"
        launched.append(line)
        return real_launch(kind, T, nt, nl, part, nparts, bucket, greedy=greedy)

    eng._launch = launch
    prompts = workload()
    params = [SamplingParams(max_tokens=int(4 + i % 9), ignore_eos=True, adapter=names[i]) for i in range(14)]
    seqs, i, it = [], 0, 0
    while i < len(prompts) or eng.has_work():
        if i < len(prompts) and it % 2 == 0:
            seqs.append(eng.add_request(prompts[i], params[i]))
            i += 1
        if it == 12:
            eng.abort(seqs[-1].seq_id)
        out = eng.step()
        kind = eng.tracer.spans[-1][0]
        outs = list(out)
        toks = " ".join(f"{o.seq_id}{'*' if o.finished else ''}" for o in outs)
        fins = " ".join(f"{o.seq_id}={o.finish_reason}" for o in outs if o.finished)
        lines.append(" || ".join([f"S {kind} {toks} | {fins}".rstrip()] + launched))
        launched.clear()
        it += 1
        assert it < 1000
    assert eng.alloc.num_free == eng.alloc.available - 1
    lines.append("F " + " ".join(f"{s.seq_id}={s.finish_reason}:{len(s.output)}" for s in seqs))
    lines.append("stats " + " ".join(f"{k}={eng.stats[k]}" for k in sorted(eng.stats) if not k.endswith(("_us", "_ms"))))
    return "\n".join(lines) + "\n"


def _write_adapters(root):
    from test_lora_cpu import write_adapter

    return {"x": write_adapter(root / "x", TINY_LLAMA, r=8, seed=11, std=0.07),
            "y": write_adapter(root / "y", TINY_LLAMA, r=4, seed=12, std=0.07, targets=("q_proj", "down_proj"))}


@pytest.fixture(scope="module")
def adapter_dirs(tmp_path_factory):
    return _write_adapters(tmp_path_factory.mktemp("adapters"))


@pytest.fixture(scope="module")
def pinned():
    runs, name = {}, None
    with open(FIXTURE) as f:
        for line in f:
            if line.startswith("# run "):
                name = line[6:].strip()
                runs[name] = ""
            runs[name] += line
    return runs


def test_fixture_holds_exactly_the_runs(pinned):
    assert list(pinned) == list(RUNS)


@pytest.mark.parametrize("name", list(RUNS))
def test_schedule_matches_the_pinned_trace(name, pinned, adapter_dirs):
    got, want = trace(name, adapter_dirs=adapter_dirs), pinned[name]
    if got != want:
        got_l, want_l = got.splitlines(), want.splitlines()
        first = next((i for i, (a, b) in enumerate(zip(got_l, want_l)) if a != b), min(len(got_l), len(want_l)))
        pytest.fail("run %s differs from tests/fixtures/engine_schedule.txt, first at its line %d:\n"
                    "  pinned: %s\n  now:    %s" % (name, first + 1, want_l[first:first + 1], got_l[first:first + 1]))


@pytest.mark.parametrize("name", ["async", "sync_mixed", "async_graphs"])
def test_trace_does_not_depend_on_the_model_seed(name, pinned):
    """No line depends on a sampled token's value: other weights, other tokens, the same trace."""
    assert trace(name, seed=2) == pinned[name]


def _stats(text):
    (line,) = [ln for ln in text.splitlines() if ln.startswith("stats ")]
    return dict(kv.split("=") for kv in line.split()[1:])


def _launches(text):
    return [rec.split() for ln in text.splitlines() if ln.startswith("S ") for rec in ln.split(" || ")[1:]]


def test_the_workload_reaches_every_kind_of_step(pinned):
    """Conditions on the workload, not measurements: without them the trace pins nothing."""
    for name in ("async", "sync_mixed", "sync_split"):
        st, text = _stats(pinned[name]), pinned[name]
        assert int(st["preemptions"]) >= 1, name
        assert int(st["prefix_hit_tokens"]) > 0, name
        assert int(st["prefill_steps"]) >= 1 and "\nS prefill" in text, name        # a prompt-only step
        assert int(st["eager_decode_steps"]) >= 1 and "\nS decode" in text, name    # an eager decode step
        assert "=abort" in text, name
        assert (int(st.get("mixed_steps", 0)) >= 1) == (name != "sync_split"), name
        assert ("\nS mixed" in text) == (name != "sync_split"), name
    # one-step-ahead: decode ids gathered on the device; never in the synchronous engine
    assert any(f[10] != "ids=-" for f in _launches(pinned["async"]))
    assert all(f[10] == "ids=-" for f in _launches(pinned["sync_mixed"]))
    # the sliding-window run releases pages, the LoRA runs launch adapter steps, the stand-in
    # graphs are replayed (bucketed launches)
    assert int(_stats(pinned["async_swa16"])["kv_pages_released"]) > 0
    for name in ("async_lora", "sync_mixed_lora"):
        assert int(_stats(pinned[name])["lora_steps"]) > 0
        assert any(f[11] == "lora=1" for f in _launches(pinned[name]))
    for name in ("async_graphs", "sync_mixed_graphs"):
        st = _stats(pinned[name])
        assert int(st["graph_steps"]) > 0
        assert any(f[1] == "2" and f[7] != "0" for f in _launches(pinned[name]))


if __name__ == "__main__":
    if sys.argv[1:] != ["--write"]:
        sys.exit("usage: python tests/test_engine_schedule_cpu.py --write")
    import pathlib
    import tempfile

    sys.path.insert(0, os.path.join(ROOT, "tests"))
    with tempfile.TemporaryDirectory() as tmp:
        dirs = _write_adapters(pathlib.Path(tmp))
        text = "".join(trace(name, adapter_dirs=dirs) for name in RUNS)
    with open(FIXTURE, "w") as f:
        f.write(text)
    print(f"wrote {FIXTURE}: {len(text.splitlines())} lines")
