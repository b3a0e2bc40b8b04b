"""Every route class of the pinned planner table (tests/gemm_probes.py: the serving block of
tests/fixtures/gemm_routes_gfx950.txt) run on the device at the class's first and last row
count, through the raw ops with no knob touched, against the exact probes.  Each case first
compares the LIVE route of its shape with the table's class, so every numerical check is known
to have run the kernel the table names; a device with another CU count than the table's skips.

(The file's name sorts it behind test_custom_ar_gpu.py on purpose, as test_probes_attention_gpu.py's
does: see the last section of profiles/attention_probes.md.)"""
import pytest
import torch

import gemm_probes as gp
from test_kernels_gpu import ROUTE_FIELDS

pytestmark = pytest.mark.gpu
TABLE_CUS = 256


@pytest.fixture(scope="module")
def be(gpu):
    cus = torch.cuda.get_device_properties(gpu).multi_processor_count
    if cus != TABLE_CUS:
        pytest.skip(f"the pinned route table is for {TABLE_CUS} CUs, this device has {cus}")
    return gp.HipBackend(gpu)


def live_route(case):
    return dict(zip(ROUTE_FIELDS, torch.ops.mlop.gemm_route(*gp.route_call(case))))


def run(case, be, gpu):
    """The probe's messages and figures.  A device fault poisons the process for every later
    launch, so it ends the session instead of failing the remaining cases one by one."""
    info = {}
    try:
        msgs = gp.probe(case, be, gpu, info)
        torch.cuda.synchronize()
    except RuntimeError as e:
        if "HIP error" in str(e) or "hipError" in str(e):
            pytest.exit(f"device fault in {case.id}: {e}", returncode=3)
        raise
    print(case.id, {k: v for k, v in info.items() if k != "out"})
    # the conditions that keep the probe sensitive, from the reference alone
    assert info["over256"] <= 0.01, (case.id, info)
    assert info.get("silu_in_range", 1.0) >= 0.95, (case.id, info)
    return msgs, info


@pytest.mark.parametrize("case", gp.CASES, ids=[c.id for c in gp.CASES])
def test_route_class(be, gpu, case):
    live = live_route(case)
    assert gp.route_class(case.op, case.K, live) == case.cls, \
        f"{case.id}: the live route {live} is not the table's class {case.cls}"
    msgs, _ = run(case, be, gpu)
    assert not msgs, "\n".join(msgs)


@pytest.mark.parametrize("case", gp.OP8_CASES, ids=[c.id for c in gp.OP8_CASES])
def test_row_scaled_plain(be, gpu, case):
    """Op 8 (ops.gemm_rs with no epilogue) is in no model's shape list, so not in the table."""
    live = live_route(case)
    assert gp.FAMILY[live["family"]] == case.cls[1], (case.id, live)
    msgs, _ = run(case, be, gpu)
    assert not msgs, "\n".join(msgs)


def _first(pred):
    return min((c for c in gp.CASES if pred(c)), key=gp.madds)


@pytest.mark.parametrize("case", [_first(lambda c: c.cls[1] == "P" and c.cls[7] > 0 and c.op == gp.PLAIN),
                                  _first(lambda c: c.op == gp.GROUPED and c.cls[1:4] == ("T", 13, 2))],
                         ids=lambda c: c.id)
def test_three_launches_bit_identical(be, gpu, case):
    """A stream-K tail and a grouped split-K launch three times in a row under default knobs:
    the tickets re-arm, the results repeat bit for bit."""
    assert gp.route_class(case.op, case.K, live_route(case)) == case.cls
    outs = []
    for _ in range(3):
        msgs, info = run(case, be, gpu)
        assert not msgs, "\n".join(msgs)
        outs.append(info["out"])
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
