"""CPU checks of the workspace protocol (include/dgv2.h "Workspaces"): every kernel whose workspace
the library sizes has one host-only `_scratch` sibling, and dgv2_native.scratch_elems is the one place that asks.  The
sizes are held to tests/golden/scratch_sizes.json, recorded before the six query modes became siblings
(tests/golden/make_scratch_golden.py).  Needs the built library, no GPU."""
import ast
import json
import os
import re

import pytest

from conftest import GOLDEN, PKG
from test_abi import HEADER, parse_header

# kernel entry -> the host-only entry that sizes its workspace
PAIRS = {
    "dgv2_conv3x3_x3_wgrad": "dgv2_conv3x3_x3_wgrad_scratch",
    "dgv2_conv_wgrad_stream_pl": "dgv2_conv_wgrad_stream_scratch",
    "dgv2_bmm_tn_stream_ld": "dgv2_bmm_tn_stream_scratch",
    "dgv2_mod_prep_all_bwd": "dgv2_mod_prep_all_bwd_scratch",
    "dgv2_pe_wgrad": "dgv2_pe_wgrad_scratch",
    "dgv2_stem_bwd_skip": "dgv2_stem_bwd_scratch",
    "dgv2_crf_rnn_backward": "dgv2_crf_rnn_backward_scratch",
    "dgv2_seg_loss_forward": "dgv2_seg_loss_scratch",
    "dgv2_fps": "dgv2_fps_scratch",
    "dgv2_resample_tab_actbwd": "dgv2_resample_tab_actbwd_scratch",
    "dgv2_fir_same_mfma_actbwd": "dgv2_fir_same_mfma_actbwd_scratch",
    "dgv2_fir_same_mfma_prep": "dgv2_fir_same_mfma_prep_scratch",
    "dgv2_bmm_nn_small_act": "dgv2_bmm_nn_small_act_scratch",
    "dgv2_head_bwd": "dgv2_head_bwd_scratch",
    "dgv2_modconv_pe_dgrad_actbwd": "dgv2_modconv_pe_dgrad_actbwd_scratch",
}
DELETED_CACHES = {"_WGRAD_SCRATCH", "_TN_SCRATCH", "_STEM_SCRATCH", "_ACTBWD_BLOCKS", "_HEAD_ACT_BLOCKS", "_DGRAD_ACT_ROWS"}
F32, BF16 = 0, 1
TN_SHAPE = (8, 64, 256, 64, 32)   # dgv2_bmm_tn_stream_scratch: the two dtypes plan different split counts here

with open(os.path.join(GOLDEN, "scratch_sizes.json")) as _f:
    ROWS = json.load(_f)


@pytest.fixture
def N():
    import dgv2_native

    saved = dict(dgv2_native._scratch_memo)
    dgv2_native._scratch_memo.clear()
    yield dgv2_native
    dgv2_native._scratch_memo.clear()
    dgv2_native._scratch_memo.update(saved)


def test_golden_covers_every_scratch_entry():
    assert {r["entry"] for r in ROWS} == set(PAIRS.values())
    for entry in PAIRS.values():
        sizes = [r["elems"] for r in ROWS if r["entry"] == entry]
        assert any(sizes), entry
        assert len(sizes) >= 2, entry


@pytest.mark.parametrize("entry", sorted(PAIRS.values()))
def test_golden_replay(N, entry):
    """The library reports what the parent commit reported (for the six new siblings: what the Python layer multiplied
    out of the kernel entry's query mode), 0 where the parent refused."""
    rows = [r for r in ROWS if r["entry"] == entry]
    for r in rows:
        assert N.scratch_elems(entry, *r["args"]) == r["elems"], r
    assert len(N._scratch_memo) == len(rows)


def test_memo_is_keyed_on_the_full_argument_list(N, monkeypatch):
    entry = "dgv2_bmm_tn_stream_scratch"
    want = {dt: next(r["elems"] for r in ROWS if r["entry"] == entry and r["args"] == [*TN_SHAPE, dt]) for dt in (F32, BF16)}
    assert want[F32] != want[BF16] and min(want.values()) > 0
    calls = []
    real = getattr(N.lib, entry)

    def counted(*a):
        calls.append(a[1:])
        return real(*a)

    monkeypatch.setattr(N.lib, entry, counted)
    for order in ((BF16, F32), (F32, BF16)):
        N._scratch_memo.clear()
        del calls[:]
        for dt in order:
            assert N.scratch_elems(entry, *TN_SHAPE, dt) == want[dt]
        assert len(N._scratch_memo) == 2 and len(calls) == 2
        for dt in order:   # the second identical call does not enter the library
            assert N.scratch_elems(entry, *TN_SHAPE, dt) == want[dt]
        assert len(N._scratch_memo) == 2 and len(calls) == 2
    # int arrays are keyed by value, whatever sequence carries them
    entry = "dgv2_mod_prep_all_bwd_scratch"
    a = N.scratch_elems(entry, [5, 3], [12, 8], 3, 2)
    assert a == N.scratch_elems(entry, (5, 3), (12, 8), 3, 2) > 0 and len(N._scratch_memo) == 3
    assert N.scratch_elems(entry, [5, 4], [12, 8], 3, 2) != a and len(N._scratch_memo) == 4


def test_return_codes(N):
    """DGV2_ENOTSUP is "no workspace / not covered" (0); every other code raises as call() does."""
    assert N.scratch_elems("dgv2_pe_wgrad_scratch", 64, 2048, 24, 512) == 0
    assert N.scratch_elems("dgv2_head_bwd_scratch", 2, 100, 5, 32, BF16) == 0
    assert N.scratch_elems("dgv2_modconv_pe_dgrad_actbwd_scratch", 64, 2048, 128, BF16) == 0
    assert N.scratch_elems("dgv2_fir_same_mfma_prep_scratch", 12, 32) == 0
    for entry, args in (("dgv2_pe_wgrad_scratch", (0, 2048, 32, 512)),
                        ("dgv2_head_bwd_scratch", (0, 100, 2, 32, BF16)),
                        ("dgv2_bmm_nn_small_act_scratch", (2, 100, 2, 32, 7)),
                        ("dgv2_resample_tab_actbwd_scratch", (0, 32, 8, 32, 2, BF16)),
                        ("dgv2_modconv_pe_dgrad_actbwd_scratch", (0, 100, 32, BF16)),
                        ("dgv2_bmm_tn_stream_scratch", (0, 64, 256, 64, 32, BF16)),
                        ("dgv2_seg_loss_scratch", (0, 9, 37))):
        with pytest.raises(RuntimeError, match=entry):
            N.scratch_elems(entry, *args)
        assert (entry, args) not in N._scratch_memo
    for entry in PAIRS.values():   # a NULL result pointer is an error everywhere
        ptr_t = N.SIGNATURES[entry][0]
        args = [N.int_array([8]) if t is ptr_t else 8 for t in N.SIGNATURES[entry][1:]]
        assert getattr(N.lib, entry)(None, *args) == -1, entry


def test_header_declares_one_sibling_per_kernel_and_no_query_mode():
    protos = parse_header()
    for kernel, sibling in PAIRS.items():
        assert kernel in protos and sibling in protos, (kernel, sibling)
        assert protos[sibling][0] == "ptr" and set(protos[sibling][1:]) <= {"int", "ptr"}, sibling
    declared = {n for n in protos if n.endswith("_scratch")}
    assert declared == set(PAIRS.values()), declared ^ set(PAIRS.values())
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    params = [p.split()[-1].lstrip("*") for m in re.finditer(r"\bint\s+dgv2_\w+\s*\(([^;]*?)\)\s*;", src, flags=re.S)
              for p in m.group(1).split(",") if p.strip() not in ("", "void")]
    assert len(params) > 1000
    assert not [p for p in params if p.endswith("_needed")]


def test_deleted_caches_stay_deleted():
    """No submodule of gans.models.ops.native binds one of the six per-site size caches again."""
    native_dir = os.path.join(PKG, "gans", "models", "ops", "native")
    files = sorted(f for f in os.listdir(native_dir) if f.endswith(".py"))
    assert len(files) >= 20
    for f in files:
        with open(os.path.join(native_dir, f)) as fh:
            tree = ast.parse(fh.read())
        bound = {n.id for n in ast.walk(tree) if isinstance(n, ast.Name) and isinstance(n.ctx, ast.Store)}
        bound |= {a.asname or a.name for n in ast.walk(tree) if isinstance(n, (ast.Import, ast.ImportFrom)) for a in n.names}
        assert not bound & DELETED_CACHES, (f, bound & DELETED_CACHES)
