"""The MoE probes of tests/moe_probes.py on the device, through the raw ops: exact expert ids
under planted ties, the dispatch layout from its definition, the grouped gate_up GEMM read
through ``a_rows`` at every grouped route class of the pinned planner table, and the tail at
every grouped down class - with y left NaN exactly where the table's route splits K, which
is the evidence that the slab-summing template of the tail ran.  No knob is touched except
``moe_mid_tok``, which the mid dispatch cases set and restore.

(The file's name sorts it behind test_custom_ar_gpu.py on purpose, as test_probes_gemm_gpu.py's
does: see the last section of profiles/attention_probes.md.)"""
import pytest
import torch

import gemm_probes as gp
import moe_probes as mp

pytestmark = pytest.mark.gpu
TABLE_CUS = 256


@pytest.fixture(scope="module")
def be(gpu):
    return mp.HipMoe(gpu)


@pytest.fixture(scope="module")
def table_be(be, gpu):
    cus = torch.cuda.get_device_properties(gpu).multi_processor_count
    if cus != TABLE_CUS:
        pytest.skip(f"the pinned route table is for {TABLE_CUS} CUs, this device has {cus}")
    return be


def run(probe, name, *args, **kw):
    """The probe's messages and figures.  A device fault poisons the process for every later
    launch, so it ends the session instead of failing the remaining cases one by one."""
    info = {}
    try:
        msgs = probe(*args, info=info, **kw)
        torch.cuda.synchronize()
    except RuntimeError as e:
        if "HIP error" in str(e) or "hipError" in str(e):
            pytest.exit(f"device fault in {name}: {e}", returncode=3)
        raise
    print(name, {k: v for k, v in info.items() if k != "counts"})
    # the conditions that keep the probe sensitive, from the reference alone
    assert info.get("over256", 0.0) <= 0.01 and info.get("silu_in_range", 1.0) >= 0.95, (name, info)
    assert info.get("logit_max", 0.0) <= mp.LOGIT_MAX, (name, info)
    assert info.get("near_tie_tokens", 0.0) <= mp.NEAR_TIE_CAP, (name, info)
    return msgs, info


def _id(v):
    return v.id if hasattr(v, "id") else "-".join(map(str, v)) if isinstance(v, tuple) else str(v)


@pytest.mark.parametrize("pro", [False, True], ids=["x", "pro"])
@pytest.mark.parametrize("shape", mp.SMALL, ids=_id)
def test_dispatch_small(be, gpu, shape, pro):
    msgs = []
    for rng in mp.RANGES:
        msgs += run(mp.probe_dispatch, f"small {shape} {rng}", "small", shape, rng, be, gpu, pro=pro)[0]
    assert not msgs, "\n".join(msgs)


@pytest.mark.parametrize("tok", mp.MID_TOKS)
@pytest.mark.parametrize("shape", mp.MID, ids=_id)
def test_dispatch_mid(be, gpu, shape, tok):
    """Every tokens-per-workgroup template (0: by T), each launched twice in a row."""
    prev = torch.ops.mlop.moe_mid_tok(-1)
    msgs = []
    try:
        assert torch.ops.mlop.moe_mid_tok(tok) == tok
        for pro in (False, True):
            for rng in mp.RANGES:
                msgs += run(mp.probe_dispatch, f"mid {shape} tok {tok} {rng}", "mid", shape, rng, be, gpu, pro=pro)[0]
    finally:
        torch.ops.mlop.moe_mid_tok(prev)
    assert not msgs, "\n".join(msgs)


@pytest.mark.parametrize("shape", mp.ROUTE, ids=_id)
def test_route_and_permute(be, gpu, shape):
    msgs = []
    for rng in mp.RANGES:
        msgs += run(mp.probe_route_permute, f"route {shape} {rng}", shape, rng, be, gpu)[0]
    assert not msgs, "\n".join(msgs)


def test_permute_by_destination_rank(be, gpu):
    msgs, _ = run(mp.probe_permute_ranks, "permute by rank", be, gpu)
    assert not msgs, "\n".join(msgs)


@pytest.mark.parametrize("case", mp.GROUPED_CASES, ids=_id)
def test_grouped_gemm_through_a_rows(be, gpu, case):
    """An indirect call's route cannot be asked through gemm_route (there is no grouped GEMV for
    it): only the numbers are asserted.  Both forms: every row valid, and a third of them not."""
    msgs = run(mp.probe_a_rows, case.id, case, be, gpu)[0]
    if mp.K_SLOTS * case.M >= 10:
        msgs += run(mp.probe_a_rows, case.id + " partial", case, be, gpu, partial=True)[0]
    assert not msgs, "\n".join(msgs)


@pytest.mark.parametrize("shape", mp.COMBINE, ids=_id)
def test_combine(be, gpu, shape):
    msgs, _ = run(mp.probe_combine, f"combine {shape}", shape, be, gpu)
    assert not msgs, "\n".join(msgs)


@pytest.mark.parametrize("shape", mp.COMBINE_NORM + [mp.COMBINE_NORM_REFUSED], ids=_id)
def test_combine_add_rmsnorm(be, gpu, shape):
    msgs, _ = run(mp.probe_combine_norm, f"combine_norm {shape}", shape, be, gpu)
    assert not msgs, "\n".join(msgs)


DOWN = [(c, False) for c in mp.DOWN_CASES] + [(c, True) for c in mp.DOWN_PARTIAL]


@pytest.mark.parametrize("case,partial", DOWN, ids=[c.id + ("-part" if p else "") for c, p in DOWN])
def test_down_combine_add_rmsnorm(table_be, gpu, case, partial):
    msgs, info = run(mp.probe_down, case.id, case, table_be, gpu, partial=partial)
    assert not msgs, "\n".join(msgs)
    assert info["y_formed"] == (not mp.is_slab(case)), (case.id, info)
