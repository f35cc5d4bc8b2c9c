"""CPU: the host layer in front of the flash-attention kernels (open_sora_amd/csrc/attention_fwd.hip).

Status table: the three entry points check their arguments before any HIP call, so a malformed call returns a status and launches
nothing -- no GPU needed.  Every call here carries at least one fault (fake, aligned addresses are never dereferenced); the
well-formed tuple itself is never passed.  One fault: the status is part of the entry point's behaviour (OSK_EINVAL = -1 for a
malformed call, OSK_EUNSUPPORTED = -2 for a well-formed one without a kernel).  Several faults: OSK_EINVAL wins.

Launch selection: osk_attention_launch_shape / osk_attention_tail_split_factor / osk_attention_body_name answer as recorded in
tests/golden/attention_launch_shapes.json (tools/make_golden_attention_launch_shapes.py; 256 CUs assumed without a device)."""
import json
import math
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EUNSUPPORTED = -1, -2

# well-formed arguments, in the order of include/osk.h.  B = 2, H = 2, head_dim 72 (every entry point has it): row stride H * hd = 144
_HEAD = dict(q=0x1000, q_batch_stride=130 * 144, q_row_stride=144, k=0x2000, k_seg_stride=64 * 144, k_batch_stride=64 * 144,
             k_row_stride=144, vt=0x3000, vt_seg_stride=2 * 72 * 64)
_MID = dict(out=0x4000, o_batch_stride=130 * 144, o_row_stride=144, lse=0x5000, B=2, H=2, Lq=130, n_seg=1, seg_len=64, hd=72,
            scale=0.125, q_prescaled=1, kv_batches=0)
_TAIL = dict(workspace=0x8000, workspace_bytes=1 << 20, stream=None)
GOOD = {
    "osk_attention_fwd_bounded_bf16": {**_HEAD, **_MID, "score_bound": 12.0, **_TAIL},
    "osk_attention_fwd_auto_bf16": {**_HEAD, **_MID, "q_norm2_max": 0x6000, "k_norm2_max": 0x7000, **_TAIL},
    "osk_attention_fwd_pv8_bf16": {**_HEAD, "v_scale": 0x6000, **_MID, **_TAIL},
}
BOUNDED, AUTO, PV8 = GOOD


def _faults(entry):
    """(what is broken, {argument: value}, expected status): exactly one fault each"""
    g = GOOD[entry]
    ptrs = ["q", "k", "vt", "out"] + {BOUNDED: [], AUTO: ["q_norm2_max", "k_norm2_max"], PV8: ["v_scale"]}[entry]   # (lse and workspace are optional)
    rows = [(f"{n} null", {n: None}, EINVAL) for n in ptrs]
    rows += [(f"{n} = 0", {n: 0}, EINVAL) for n in ("B", "H", "Lq", "n_seg", "seg_len")]
    # strides: off by the largest power of two below the granularity (8 bf16 elements; 4 for the output; 16 bytes for the e4m3 V^T)
    off = dict(q_batch_stride=4, q_row_stride=4, k_seg_stride=4, k_batch_stride=4, k_row_stride=4, vt_seg_stride=4, o_batch_stride=2, o_row_stride=2)
    if entry == PV8:
        off["vt_seg_stride"] = 8      # legal for a bf16 V^T, illegal for the byte layout
    rows += [(f"{n} off its mask", {n: g[n] + d}, EINVAL) for n, d in off.items()]
    mis = dict(q=8, k=8, vt=8, out=4)
    if entry == AUTO:
        mis.update(q_norm2_max=2, k_norm2_max=2)
    rows += [(f"{n} misaligned", {n: g[n] + d}, EINVAL) for n, d in mis.items()]
    rows += [("kv_batches = -1", {"kv_batches": -1}, EINVAL), ("kv_batches = B + 1", {"kv_batches": g["B"] + 1}, EINVAL),
             ("workspace misaligned", {"workspace": g["workspace"] + 8}, EINVAL), ("workspace_bytes < 0", {"workspace_bytes": -1}, EINVAL)]
    if entry == BOUNDED:
        rows += [("score_bound = -1", {"score_bound": -1.0}, EINVAL), ("score_bound NaN", {"score_bound": math.nan}, EINVAL)]
    if entry == AUTO:
        rows += [("scale not folded into q", {"q_prescaled": 0, "scale": 0.125}, EUNSUPPORTED)]   # 0.125 log2(e) != 1
    rows += [("hd = 48", {"hd": 48}, EUNSUPPORTED)]
    if entry == PV8:
        rows += [("hd = 64", {"hd": 64}, EUNSUPPORTED)]
    return rows


SINGLE = [pytest.param(e, chg, st, id=f"{e[len('osk_attention_fwd_'):-len('_bf16')]}: {what}") for e in GOOD for what, chg, st in _faults(e)]
# a malformed call that also asks for an uncompiled head dim (or breaks auto's scale rule) is reported as malformed
DOUBLE = [
    pytest.param(BOUNDED, {"hd": 48, "score_bound": -1.0}, id="bounded: hd = 48 and score_bound = -1"),
    pytest.param(AUTO, {"hd": 48, "kv_batches": -1}, id="auto: hd = 48 and kv_batches = -1"),
    pytest.param(AUTO, {"q_prescaled": 0, "scale": 0.125, "workspace_bytes": -1}, id="auto: scale not folded and workspace_bytes < 0"),
    pytest.param(PV8, {"hd": 64, "workspace": 0x8008}, id="pv8: hd = 64 and workspace misaligned"),
]


def _call(entry, changes):
    from open_sora_amd import _C

    assert changes, "the well-formed tuple is never passed: it would launch"
    args = {**GOOD[entry], **changes}
    assert list(args) == list(GOOD[entry])
    return getattr(_C.lib, entry)(*args.values())


@pytest.mark.parametrize("entry, changes, status", SINGLE)
def test_single_fault_status(entry, changes, status):
    assert _call(entry, changes) == status


@pytest.mark.parametrize("entry, changes", DOUBLE)
def test_einval_comes_before_eunsupported(entry, changes):
    assert _call(entry, changes) == EINVAL


def test_launch_selection_matches_the_recorded_fixture():
    from open_sora_amd import _C

    assert not torch.cuda.is_available() or torch.cuda.get_device_properties(0).multi_processor_count == 256, \
        "the fixture was recorded for 256 CUs (an MI355X, or no device)"
    with open(os.path.join(ROOT, "tests", "golden", "attention_launch_shapes.json")) as f:
        gold = json.load(f)
    ws_bytes = _C.lib.osk_attention_workspace_bytes()
    assert ws_bytes == gold["workspace_bytes"]
    shapes, grid = gold["shapes"], gold["grid"]
    assert len(shapes) >= 300
    for col, name in enumerate(("hd", "B", "H", "Lq")):          # every value of every axis is met
        assert {r[col] for r in shapes} == set(grid[name]), name
    assert {(r[4], r[5]) for r in shapes} == {tuple(s) for s in grid["segments"]}
    assert {r[6] for r in shapes} == set(grid["bound"]) and {r[7] for r in shapes} == {0, 1}
    bad = []
    for hd, B, H, Lq, n_seg, seg_len, bound, ws, parts, rows, split in shapes:
        got = (*_C.attention_launch_shape(B, H, Lq, n_seg, seg_len, hd, bound, ws * ws_bytes),
               _C.lib.osk_attention_tail_split_factor(B, H, Lq, n_seg, seg_len, hd, ws * ws_bytes))
        if got != (parts, rows, split):
            bad.append(((hd, B, H, Lq, n_seg, seg_len, bound, ws), got, (parts, rows, split)))
    assert not bad, bad[:5]
    assert len(gold["bodies"]) == len(grid["hd"]) * len(grid["segments"]) * len(grid["bound"])
    for hd, n_seg, seg_len, bound, body in gold["bodies"]:
        assert _C.attention_body(hd, n_seg, seg_len, bound) == body, (hd, n_seg, seg_len, bound)
