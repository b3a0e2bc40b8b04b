"""The sampler probes of tests/sampler_probes.py on the device: every launch through
``ops.sample`` (or ``Sampler.__call__`` for the seeded, mixed batches), three times in a row;
every row's token must EQUAL the fp64 oracle's - no neighbour allowance, no eps - and the three
outputs must be identical.  The margin that makes equality a fair demand is asserted from the
reference alone, before the comparison.

(The file's name sorts it behind test_custom_ar_gpu.py on purpose, as test_probes_gemm_gpu.py's
does: see the last section of profiles/attention_probes.md.)"""
import pytest
import torch

import sampler_probes as sp

pytestmark = pytest.mark.gpu


def run(la, device):
    """The probe's messages and figures.  A device fault poisons the process for every later
    launch, so it ends the session instead of failing the remaining cases one by one."""
    info = {}
    try:
        msgs = sp.probe(la, device=device, info=info)
        torch.cuda.synchronize()
    except RuntimeError as e:
        if "HIP error" in str(e) or "hipError" in str(e):
            pytest.exit(f"device fault in {la.name}: {e}", returncode=3)
        raise
    print(la.name, info)
    return msgs, info


@pytest.mark.parametrize("name", sp.NAMES)
def test_tokens_equal_the_oracle(gpu, name):
    la = sp.launch(name)
    msgs, info = run(la, gpu)
    assert info["margin_ok"] and info["min_margin"] >= sp.MARGIN, (name, info)
    assert not msgs, "\n".join(msgs)
