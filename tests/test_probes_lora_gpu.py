"""Every case of tests/lora_probes.py on the device, through the raw ops: the shrink in every form
of its K loop, the expand at every R, tiles that mix up to 16 slots.  No case is sampled, and no
comparison has a tolerance.  profiles/lora_probes.md has the measured figures (each test prints
its own: ``pytest -s``).

(The file's name sorts it behind test_custom_ar_gpu.py on purpose, as the other probe files' do:
see the last section of profiles/attention_probes.md.)"""
import pytest
import torch

import lora_probes as lp

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def be(gpu):
    return lp.HipBackend(gpu)


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
    print(what, info)
    return msgs


@pytest.mark.parametrize("case", lp.SHRINK_CASES, ids=[c.id for c in lp.SHRINK_CASES])
def test_shrink(be, gpu, case):
    msgs = []
    for name, fn in lp.SHRINK_PROBES.items():
        msgs += run(f"{case.id} {name} ({lp.form_name(case.K)})", fn, case, be, gpu)
    assert not msgs, "\n".join(msgs)


@pytest.mark.parametrize("case", lp.EXPAND_CASES, ids=[c.id for c in lp.EXPAND_CASES])
def test_expand_add(be, gpu, case):
    msgs = []
    for name, fn in lp.EXPAND_PROBES.items():
        msgs += run(f"{case.id} {name} {lp.expand_blocks(case.N)}", fn, case, be, gpu)
    assert not msgs, "\n".join(msgs)


@pytest.mark.parametrize("case", lp.CHAIN_CASES, ids=[c.id for c in lp.CHAIN_CASES])
def test_shrink_into_expand(be, gpu, case):
    msgs = run(case.id, lp.probe_chain, case, be, gpu)
    assert not msgs, "\n".join(msgs)


def test_no_tokens(be, gpu):
    try:
        msgs = lp.probe_empty(be, gpu)
        torch.cuda.synchronize()
    except RuntimeError as e:
        if "HIP error" in str(e) or "hipError" in str(e):
            pytest.exit(f"device fault in the 0-token launches: {e}", returncode=3)
        raise
    assert not msgs, "\n".join(msgs)
