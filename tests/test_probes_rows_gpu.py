"""Every case of tests/row_probes.py on the device, through the raw ops: RMSNorm and add+RMSNorm
in every launch form, SiLU-mul in both layouts, the embedding gather, and the bf16 and fp8 RoPE +
paged-cache writers.  No case is sampled.  profiles/row_probes.md has the measured figures
(each test prints its own: ``pytest -s``).

(The file's name sorts it behind test_custom_ar_gpu.py on purpose, as the other probe files' do:
see the last section of profiles/attention_probes.md.)"""
import pytest
import torch

import row_probes as rp

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def be(gpu):
    return rp.HipBackend(gpu)


def run(what, fn, *args):
    """The probe's messages and figures.  A device fault poisons the process for every later
    launch, so it ends the session instead of failing the remaining cases one by one."""
    info = {}
    try:
        msgs = fn(*args, info)
        torch.cuda.synchronize()
    except RuntimeError as e:
        if "HIP error" in str(e) or "hipError" in str(e):
            pytest.exit(f"device fault in {what}: {e}", returncode=3)
        raise
    print(what, {k: v for k, v in info.items() if k != "placed"})
    assert info.get("either", 0.0) <= 0.01, (what, info)  # the reference's own condition
    return msgs, info


@pytest.mark.parametrize("case", rp.NORM_CASES, ids=[c.id for c in rp.NORM_CASES])
def test_norm(be, gpu, case):
    msgs = []
    for name in rp.norm_probes_of(case):
        msgs += run(f"{case.id} {name} {rp.norm_form(case.M, case.H)}", rp.NORM_PROBES[name], case, be, gpu)[0]
    assert not msgs, "\n".join(msgs)


@pytest.mark.parametrize("case", rp.SILU_CASES, ids=[c.id for c in rp.SILU_CASES])
def test_silu_mul(be, gpu, case):
    msgs = []
    for name, fn in rp.SILU_PROBES.items():
        m, info = run(f"{case.id} {name}", fn, case, be, gpu)
        msgs += m
        if name == "gates" and case.M * case.I >= rp.N_FINITE:
            assert info["gates"] == rp.N_FINITE
    assert not msgs, "\n".join(msgs)


def test_silu_mul_refuses_an_interleaved_width_without_whole_groups(be, gpu):
    """I = 40 (I / 8 odd) runs in the plain layout only: the last 16-group of the interleaved one
    would lie past the row."""
    M, I = rp.SILU_REFUSED
    out = rp._padded(M, I, gpu)
    with pytest.raises(RuntimeError, match="multiple of 16/32"):
        be.silu_mul(out[:M], torch.zeros(M, 2 * I, dtype=torch.bfloat16, device=gpu), 1)
    assert bool((out == rp.SENTINEL).all())


@pytest.mark.parametrize("case", rp.EMB_CASES, ids=[c.id for c in rp.EMB_CASES])
def test_embedding(be, gpu, case):
    msgs, _ = run(case.id, rp.probe_embedding, case, be, gpu)
    assert not msgs, "\n".join(msgs)


@pytest.mark.parametrize("case", rp.ROPE_CASES, ids=[c.id for c in rp.ROPE_CASES])
def test_rope_cache_selector_table(be, gpu, case):
    msgs, _ = run(f"{case.id} {rp.rope_blocks(case)}", rp.probe_rope, case, be, gpu)
    assert not msgs, "\n".join(msgs)


@pytest.mark.parametrize("case", rp.REAL_CASES, ids=[c.id for c in rp.REAL_CASES])
def test_rope_cache_real_table(be, gpu, case):
    msgs, _ = run(case.id, rp.probe_rope_real, case, be, gpu)
    assert not msgs, "\n".join(msgs)


@pytest.mark.parametrize("add", [False, True], ids=["rmsnorm", "add_rmsnorm"])
def test_norm_of_no_rows(be, gpu, add):
    assert not rp.probe_norm_empty(be, gpu, add)


@pytest.mark.parametrize("interleaved", [0, 1])
def test_silu_mul_of_no_rows(be, gpu, interleaved):
    assert not rp.probe_silu_empty(be, gpu, interleaved)


def test_embedding_of_no_tokens(be, gpu):
    assert not rp.probe_embedding_empty(be, gpu)


@pytest.mark.parametrize("fp8", [0, 1], ids=["bf16", "fp8"])
def test_rope_cache_of_no_tokens(be, gpu, fp8):
    assert not rp.probe_rope_empty(be, gpu, fp8)
