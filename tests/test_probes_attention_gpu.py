"""The attention kernels against the exact probes of tests/attn_probes.py (counting: which keys
are visible; needle: which V row goes with which K, under every target schedule), at contexts
up to 1500 keys where a randn check at 2e-2 cannot see one wrong key.  Every launch writes into a
NaN-filled ``out``; padding rows must come back zero, everything else within one bf16 ulp of the
expected value, channels expected 0 exactly 0.

(The file's name sorts it behind test_custom_ar_gpu.py on purpose: that file's 8-process test
needs a pytest process that has not opened the GPU yet - see its docstring - and this file is
the first in the alphabet whose tests run kernels in the pytest process itself.)"""
import functools

import pytest
import torch

import attn_probes as ap
from mlopamd import ops
from test_attention_probes_cpu import planner_case

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=16)
def probe(device, kind, schedule, q_lens, ctx_lens, G, window=0, flash_min_q=1 << 30):
    """One probe launch on the device (one partition; repartition() gives the other forms).  The
    cases of a geometry follow each other, so a handful of entries serves the whole file."""
    return ap.build(kind, list(q_lens), list(ctx_lens), ap.HKV, G, window, flash_min_q, device=device,
                    schedule=schedule)


def launch(m, q, kc, vc, exp, what):
    out = torch.full_like(q, float("nan"))
    ops.paged_attention(q, kc, vc, m, out=out)
    assert torch.isfinite(out).all(), f"{what}: non-finite output rows"
    ap.assert_probe(out, exp, what)
    return out


def run_forms(m, q, kc, vc, exp, part_tokens, nparts, fused, what):
    """One launch of a split-KV form; the in-launch combine runs twice: its tickets must be back
    at zero after each launch and the second launch must repeat the first."""
    m = ap.repartition(m, part_tokens, nparts, sem=fused)
    outs = [launch(m, q, kc, vc, exp, what)]
    if fused:
        assert int(m.part_sem.abs().sum()) == 0, f"{what}: tickets not re-armed"
        outs.append(launch(m, q, kc, vc, exp, what + " (second launch)"))
        assert int(m.part_sem.abs().sum()) == 0, f"{what}: tickets not re-armed"
        assert torch.equal(outs[0], outs[1])


@pytest.fixture
def kv_nt(request):
    prev = torch.ops.mlop.attn_kv_nt(-1)
    torch.ops.mlop.attn_kv_nt(request.param)
    yield request.param
    torch.ops.mlop.attn_kv_nt(prev)


@pytest.mark.parametrize("kv_nt", [0, 1, 3], indirect=True)
@pytest.mark.parametrize("form", list(ap.DECODE_FORMS))
@pytest.mark.parametrize("G", ap.DECODE_G)
def test_decode(gpu, attn_fused_all, G, form, kv_nt):
    """The decode / ragged kernel, every GQA group it is compiled for (16 included), plain and
    non-temporal instantiations (>= 8 tiles: attn_kv_nt decides), one partition, 256-key partitions
    through the reduce launch and through the in-launch combine, and 32-key partitions: every
    page-pair boundary a partition boundary."""
    q_lens, ctx_lens = ap.decode_launch(G)
    part_tokens, nparts, fused = ap.DECODE_FORMS[form]
    for kind, schedule in ap.PROBES:
        m, q, kc, vc, exp = probe(str(gpu), kind, schedule, tuple(q_lens), tuple(ctx_lens), G)
        assert m.tile_seq.numel() >= 8 and m.ptile_seq.numel() == 0
        run_forms(m, q, kc, vc, exp, part_tokens, nparts, fused, f"{kind}/{schedule}")


@pytest.mark.parametrize("form", ap.WIN_FORMS)
@pytest.mark.parametrize("G", ap.WIN_DECODE_G)
@pytest.mark.parametrize("W", ap.WIN_DECODE_W)
def test_windowed_decode(gpu, attn_fused_all, W, G, form):
    """The windowed instantiations: window starts off a pair boundary, in the second page of a
    pair, on a boundary; contexts shorter than the window and 1500 keys; partitions counted from
    the window start, combined in the launch and by the reduce launch."""
    q_lens, ctx_lens = ap.windowed_decode_launch(W)
    part_tokens, nparts, fused = ap.windowed_form(form, W, G)
    for kind, schedule in ap.PROBES:
        m, q, kc, vc, exp = probe(str(gpu), kind, schedule, tuple(q_lens), tuple(ctx_lens), G, W)
        run_forms(m, q, kc, vc, exp, part_tokens, nparts, fused, f"{kind}/{schedule}")


@functools.lru_cache(maxsize=1)
def randn_case(device, G=4, seed=0):
    """Decode rows at every page / pair edge up to 300 keys, 5-token rows, a chunk that straddles
    tiles and one padding row, over randn q / K / V: partials whose every bit matters."""
    ctxs = [1, 15, 16, 17, 31, 32, 33, 127, 129, 300]
    q_lens, ctx_lens = [1] * len(ctxs) + [5, 5, 16 // G + 1, 1], ctxs + [35, 300, 260, 0]
    m = ap.make_layout(q_lens, ctx_lens, ap.HKV, G, device=device, seed=seed)
    g = torch.Generator().manual_seed(seed)
    kc, vc = (torch.randn(m.NB, ap.HKV, 16, 128, generator=g).to(torch.bfloat16).to(device) for _ in range(2))
    q = torch.randn(m.num_tokens, ap.HKV * G, 128, generator=g).to(torch.bfloat16).to(device)
    return m, q, kc, vc


@pytest.mark.parametrize("W", [0, 100, 300])
def test_fused_and_reduce_combine_bit_identical(gpu, attn_fused_all, W):
    """The in-launch combine and the reduce launch are one function over the same slabs in the
    same order, so three partitions of 128 keys (G = 4) give the same bytes either way: plain, and
    under windows that leave a row two (100) and three (300) partitions counted from its start.
    (fp8 pages: test_fp8_kv_kernels_gpu.py.)"""
    m, q, kc, vc = randn_case(str(gpu))
    outs = []
    for fused in (False, True):
        mm = ap.repartition(m, 128, 3, sem=fused)
        mm.window = W
        outs.append(ops.paged_attention(q, kc, vc, mm, out=torch.full_like(q, float("nan"))))
        assert torch.isfinite(outs[-1]).all()
    assert float(outs[0].float().abs().max()) > 0
    assert torch.equal(outs[0].view(torch.int16), outs[1].view(torch.int16))


FLASH_GRIDS = dict(grid=(0, 0), persist3=(3 * 64, 0), stream3=(3 * 64, 1), stream1=(64, 1))


@pytest.fixture
def flash_grid(request):
    """test_kernels_gpu's flash_persist: one workgroup per flash item, the persistent grid with 3
    slots per kv head per tile or as one cross-tile stream, and ONE streaming slot per kv head."""
    persist, stream = request.param
    prev, prev_s = torch.ops.mlop.flash_persist(-1), torch.ops.mlop.flash_stream(-1)
    torch.ops.mlop.flash_persist(persist)
    torch.ops.mlop.flash_stream(stream)
    yield request.param
    torch.ops.mlop.flash_persist(prev)
    torch.ops.mlop.flash_stream(prev_s)


@pytest.mark.parametrize("flash_grid", list(FLASH_GRIDS.values()), ids=list(FLASH_GRIDS), indirect=True)
@pytest.mark.parametrize("launch_id", list(ap.FLASH_LAUNCHES))
@pytest.mark.parametrize("G", ap.FLASH_G)
def test_flash(gpu, flash_grid, G, launch_id):
    """The flash-prefill kernels on every grid: fresh prompts with partial last tiles, a chunk of
    300 tokens ending at 1500 keys (with a decode row in the launch), one prompt of 1024."""
    q_lens, ctx_lens = ap.FLASH_LAUNCHES[launch_id]
    for kind, schedule in ap.PROBES:
        m, q, kc, vc, exp = probe(str(gpu), kind, schedule, tuple(q_lens), tuple(ctx_lens), G, 0, ap.FLASH_MIN_Q)
        assert m.ptile_seq.numel() > 0
        launch(m, q, kc, vc, exp, f"{kind}/{schedule}")


@pytest.mark.parametrize("G", ap.FLASH_G)
@pytest.mark.parametrize("W", ap.WIN_FLASH_W)
def test_windowed_flash(gpu, W, G):
    """Windowed flash tiles of fresh prompts and of chunks with 50 earlier tokens: windows smaller
    than a tile's token span, ring starts on every pair index mod 3."""
    q_lens, ctx_lens = ap.windowed_flash_launch()
    for kind, schedule in ap.PROBES:
        m, q, kc, vc, exp = probe(str(gpu), kind, schedule, tuple(q_lens), tuple(ctx_lens), G, W, ap.FLASH_MIN_Q)
        assert m.ptile_seq.numel() > 0 and m.tile_seq.numel() == 0
        launch(m, q, kc, vc, exp, f"{kind}/{schedule}")


@pytest.mark.parametrize("window", [0, 100])
def test_through_the_planner(gpu, window):
    """A mixed step laid out by MetaBuffers (fill_mixed, plan_partitions, meta; its own partial
    buffers and tickets), uploaded: decode rows split over partitions and a prompt chunk."""
    for kind, schedule in ap.PROBES:
        meta, q, kc, vc, exp = planner_case(kind, schedule, window, device=gpu)
        torch.cuda.synchronize()   # the metadata upload is asynchronous
        assert meta.nparts > 1 and meta.ptile_seq.numel() > 0
        launch(meta, q, kc, vc, exp, f"{kind}/{schedule}")
        assert int(meta.part_sem.abs().sum()) == 0
