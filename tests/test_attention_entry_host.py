"""CPU: the host layer in front of the flash-attention kernels (open_sora_amd/csrc/attention_fwd.hip).

Status table: the flash entry points (bounded, auto, pv8, qk8, ragged in its three operand modes, window, window_fp8 in its two) check their arguments before any HIP call, so a malformed call returns a status and launches
nothing -- no GPU needed.  Every call here carries at least one fault (fake, aligned addresses are never dereferenced); the
well-formed tuple itself is never passed.  One fault: the status is part of the entry point's behaviour (OSK_EINVAL = -1 for a
malformed call, OSK_EUNSUPPORTED = -2 for a well-formed one without a kernel).  Several faults: OSK_EINVAL wins.

Launch parameters: tests/attention_param_probe.hip, a stand-alone host program, links attention_fwd.hip against stub launch functions
and prints every AttnParams field of every launch the entry points make for a set of well-formed calls; the output is compared with
tests/golden/attention_launch_params.json field for field (tools/make_golden_attention_launch_params.py; no kernel runs).

Launch selection: osk_attention_launch_shape / osk_attention_tail_split_factor / osk_attention_body_name answer as recorded in
tests/golden/attention_launch_shapes.json (tools/make_golden_attention_launch_shapes.py; 256 CUs assumed without a device)."""
import json
import math
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EUNSUPPORTED = -1, -2

# well-formed arguments, in the order of include/osk.h.  B = 2, H = 2; head_dim 72 (every bf16 / pv8 entry point has it): row stride
# H * hd = 144; head_dim 128 for the e4m3-K (qk8) operands: row stride 256, K packed [Bkv, H, Lp, 128] with byte strides
_HEAD = dict(q=0x1000, q_batch_stride=130 * 144, q_row_stride=144, k=0x2000, k_seg_stride=64 * 144, k_batch_stride=64 * 144,
             k_row_stride=144, vt=0x3000, vt_seg_stride=2 * 72 * 64)
_MID = dict(out=0x4000, o_batch_stride=130 * 144, o_row_stride=144, lse=0x5000, B=2, H=2, Lq=130, n_seg=1, seg_len=64, hd=72,
            scale=0.125, q_prescaled=1, kv_batches=0)
_TAIL = dict(workspace=0x8000, workspace_bytes=1 << 20, stream=None)
_Q128 = dict(q_batch_stride=130 * 256, q_row_stride=256, o_batch_stride=130 * 256, o_row_stride=256, hd=128)
MODE_OF = {"bf16": 0, "pv8": 1, "qk8": 2}      # OSK_ATTN_* of include/osk.h


def _ragged(mode):
    """osk_attention_fwd_ragged_bf16: n_seg = 2 segments of 64 keys, the last holds 40"""
    k = dict(k=0x2000, k_seg_stride=2 * 64 * 144, k_batch_stride=64 * 144, k_row_stride=144, k_scale=None,
             vt=0x3000, vt_seg_stride=2 * 2 * 72 * 64, v_scale=None)
    if mode != "bf16":
        k.update(vt_seg_stride=2 * 2 * 80 * 64, v_scale=0x6000)
    if mode == "qk8":
        k.update(k_seg_stride=2 * 2 * 64 * 128, k_batch_stride=2 * 64 * 128, k_row_stride=128, k_scale=0x7000, vt_seg_stride=2 * 2 * 144 * 64)
    g = dict(q=0x1000, q_batch_stride=130 * 144, q_row_stride=144, **k, out=0x4000, o_batch_stride=130 * 144, o_row_stride=144,
             lse=0x5000, B=2, H=2, Lq=130, n_seg=2, seg_len=64, last_seg_len=40, hd=72, scale=0.125, q_prescaled=1, kv_batches=0,
             score_bound=12.0 if mode == "bf16" else 0.0, mode=MODE_OF[mode], **_TAIL)
    return {**g, **_Q128} if mode == "qk8" else g


def _window(mode):
    """osk_attention_fwd_window_bf16 / _window_fp8_bf16: Lk = 128 keys of which 64 are the prefix; one 256-row query block"""
    fp8 = mode != "bf16"
    g = dict(q=0x1000, q_batch_stride=130 * 144, q_row_stride=144, k=0x2000, k_batch_stride=128 * 144, k_row_stride=144)
    if mode == "qk8":
        g.update(k_batch_stride=2 * 128 * 128, k_row_stride=128)
    if fp8:
        g.update(k_scale=0x7000 if mode == "qk8" else None)
    g.update(vt=0x3000)
    if fp8:
        g.update(v_scale=0x6000)
    g.update(out=0x4000, o_batch_stride=130 * 144, o_row_stride=144, lse=0x5000, B=2, H=2, Lq=130, Lk=128, n_prefix=64, hd=72,
             scale=0.125, q_prescaled=1, kv_batches=0)
    g.update({"mode": MODE_OF[mode]} if fp8 else {"score_bound": 12.0})
    g.update(windows=0x9000, n_windows=1, **_TAIL)
    return {**g, **_Q128} if mode == "qk8" else g


# case -> (entry point, operand mode, well-formed arguments)
CASES = {
    "bounded": ("osk_attention_fwd_bounded_bf16", "bf16", {**_HEAD, **_MID, "score_bound": 12.0, **_TAIL}),
    "auto": ("osk_attention_fwd_auto_bf16", "bf16", {**_HEAD, **_MID, "q_norm2_max": 0x6000, "k_norm2_max": 0x7000, **_TAIL}),
    "pv8": ("osk_attention_fwd_pv8_bf16", "pv8", {**_HEAD, "v_scale": 0x6000, **_MID, **_TAIL}),
    "qk8": ("osk_attention_fwd_qk8_bf16", "qk8",
            {**dict(q=0x1000, q_batch_stride=130 * 256, q_row_stride=256, k=0x2000, k_seg_stride=2 * 2 * 64 * 128, k_batch_stride=2 * 64 * 128,
                    k_row_stride=128, k_scale=0x7000, vt=0x3000, vt_seg_stride=2 * 2 * 144 * 64, v_scale=0x6000), **_MID, **_Q128, **_TAIL}),
    "ragged bf16": ("osk_attention_fwd_ragged_bf16", "bf16", _ragged("bf16")),
    "ragged pv8": ("osk_attention_fwd_ragged_bf16", "pv8", _ragged("pv8")),
    "ragged qk8": ("osk_attention_fwd_ragged_bf16", "qk8", _ragged("qk8")),
    "window": ("osk_attention_fwd_window_bf16", "bf16", _window("bf16")),
    "window_fp8 pv8": ("osk_attention_fwd_window_fp8_bf16", "pv8", _window("pv8")),
    "window_fp8 qk8": ("osk_attention_fwd_window_fp8_bf16", "qk8", _window("qk8")),
}
BOUNDED, AUTO, PV8, QK8 = list(CASES)[:4]


def _merge_bytes(g):
    """(f32 partials of the second launch, the lse the ragged / window entries borrow when the caller keeps none), as include/osk.h states them"""
    return (g["Lq"] + 255) // 256 * g["B"] * g["H"] * 256 * (g["hd"] + 1) * 4, (g["B"] * g["H"] * g["Lq"] * 4 + 15) // 16 * 16


def _faults(case):
    """(what is broken, {argument: value}, expected status): exactly one fault each"""
    _, mode, g = CASES[case]
    ragged, window = case.startswith("ragged"), case.startswith("window")
    merges = ragged or window                 # a second launch into f32 partials + the in-place merge: workspace and 16-byte `out` rows
    scales = {"bf16": [], "pv8": ["v_scale"], "qk8": ["k_scale", "v_scale"]}[mode]
    ptrs = ["q", "k", "vt", "out"] + (["q_norm2_max", "k_norm2_max"] if case == AUTO else scales) + (["windows"] if window else [])
    rows = [(f"{n} null", {n: None}, EINVAL) for n in ptrs]                       # (lse is optional; so is the workspace of a plain call)
    rows += [(f"{n} = 0", {n: 0}, EINVAL) for n in ("B", "H", "Lq", "n_seg", "seg_len", "Lk") if n in g]
    # strides: off by the largest power of two below the granularity (8 bf16 elements; 4 for the output; 16 bytes for the e4m3 K and V^T)
    off = dict(q_batch_stride=4, q_row_stride=4, k_seg_stride=4, k_batch_stride=4, k_row_stride=4, vt_seg_stride=4, o_batch_stride=2, o_row_stride=2)
    if mode != "bf16":
        off["vt_seg_stride"] = 8      # legal for a bf16 V^T, illegal for the byte layout
    if mode == "qk8":
        off.update(k_seg_stride=8, k_batch_stride=8)
    if merges:
        off.update(o_batch_stride=4, o_row_stride=4)      # legal for a plain call; the merge reads and writes 16-byte pieces
    rows += [(f"{n} off its mask", {n: g[n] + d}, EINVAL) for n, d in off.items() if n in g]
    mis = dict(q=8, k=8, vt=8, out=8 if merges else 4)
    if case == AUTO:
        mis.update(q_norm2_max=2, k_norm2_max=2)
    if case != PV8:                   # (osk_attention_fwd_pv8_bf16 checks v_scale for null only: DIFFER below)
        mis.update({n: 2 for n in scales})
    if window:
        mis["windows"] = 2
    rows += [(f"{n} misaligned", {n: g[n] + d}, EINVAL) for n, d in mis.items()]
    rows += [("kv_batches = -1", {"kv_batches": -1}, EINVAL), ("kv_batches = B + 1", {"kv_batches": g["B"] + 1}, EINVAL),
             ("workspace misaligned", {"workspace": g["workspace"] + 8}, EINVAL), ("workspace_bytes < 0", {"workspace_bytes": -1}, EINVAL)]
    if "score_bound" in g:
        rows += [("score_bound = -1", {"score_bound": -1.0}, EINVAL), ("score_bound NaN", {"score_bound": math.nan}, EINVAL)]
    if case == AUTO:
        rows += [("scale not folded into q", {"q_prescaled": 0, "scale": 0.125}, EUNSUPPORTED)]   # 0.125 log2(e) != 1
    if mode == "qk8":
        rows += [(f"{n} < 0", {n: -g[n]}, EINVAL) for n in ("k_seg_stride", "k_batch_stride") if n in g]
        rows += [("k_row_stride = 136", {"k_row_stride": 136}, EUNSUPPORTED)]      # well-formed, but not the packed layout
    if "mode" in g:
        rows += [("mode = -1", {"mode": -1}, EINVAL), ("mode = 3", {"mode": 3}, EINVAL)]
        if window:
            rows += [("mode = OSK_ATTN_BF16", {"mode": 0}, EINVAL)]
    if ragged:
        rows += [("n_seg = 1", {"n_seg": 1}, EINVAL), ("last_seg_len = 0", {"last_seg_len": 0}, EINVAL),
                 ("last_seg_len > seg_len", {"last_seg_len": g["seg_len"] + 1}, EINVAL)]
    if window:
        rows += [("n_windows = 0", {"n_windows": 0}, EINVAL), ("n_windows = 2", {"n_windows": 2}, EINVAL),
                 ("n_prefix = 32", {"n_prefix": 32}, EINVAL), ("n_prefix = -64", {"n_prefix": -64}, EINVAL),
                 ("n_prefix = Lk", {"n_prefix": g["Lk"]}, EINVAL), ("n_prefix > Lk", {"n_prefix": g["Lk"] + 64}, EINVAL)]
    if merges:
        part, lse = _merge_bytes(g)
        rows += [("workspace null", {"workspace": None}, EINVAL), ("workspace one byte short", {"workspace_bytes": part - 1}, EINVAL),
                 ("no lse and no room to borrow one", {"lse": None, "workspace_bytes": part + lse - 1}, EINVAL)]
    rows += [(f"hd = {hd}", {"hd": hd}, EUNSUPPORTED) for hd in {"bf16": [48], "pv8": [48, 64], "qk8": [48, 64, 72]}[mode]]
    return rows


SINGLE = [pytest.param(c, chg, st, id=f"{c}: {what}") for c in CASES for what, chg, st in _faults(c)]
# a malformed call that also asks for an uncompiled head dim (or breaks auto's scale rule) is reported as malformed
DOUBLE = [
    pytest.param(BOUNDED, {"hd": 48, "score_bound": -1.0}, id="bounded: hd = 48 and score_bound = -1"),
    pytest.param(AUTO, {"hd": 48, "kv_batches": -1}, id="auto: hd = 48 and kv_batches = -1"),
    pytest.param(AUTO, {"q_prescaled": 0, "scale": 0.125, "workspace_bytes": -1}, id="auto: scale not folded and workspace_bytes < 0"),
    pytest.param(PV8, {"hd": 64, "workspace": 0x8008}, id="pv8: hd = 64 and workspace misaligned"),
    pytest.param(QK8, {"hd": 72, "k_row_stride": 136, "k_scale": 0x7002}, id="qk8: hd = 72, k_row_stride = 136 and k_scale misaligned"),
    pytest.param("ragged bf16", {"hd": 48, "last_seg_len": 65}, id="ragged bf16: hd = 48 and last_seg_len > seg_len"),
    pytest.param("ragged pv8", {"hd": 64, "workspace": None}, id="ragged pv8: hd = 64 and workspace null"),
    pytest.param("ragged qk8", {"k_row_stride": 136, "k_batch_stride": 2 * 64 * 128 + 8}, id="ragged qk8: k_row_stride = 136 and k_batch_stride off 16"),
    pytest.param("window", {"hd": 48, "n_prefix": 32}, id="window: hd = 48 and n_prefix = 32"),
    pytest.param("window_fp8 pv8", {"hd": 64, "out": 0x4008}, id="window_fp8 pv8: hd = 64 and out misaligned"),
    pytest.param("window_fp8 qk8", {"k_row_stride": 136, "n_windows": 2}, id="window_fp8 qk8: k_row_stride = 136 and n_windows = 2"),
]
# where the entries differ today: osk_attention_fwd_pv8_bf16 checks v_scale for null only, every other fp8 entry for 4-byte alignment too
# (shown beside an uncompiled head dim, so that no call is well-formed: the entry that does not check reports the head dim)
DIFFER = [
    pytest.param(PV8, {"v_scale": 0x6002, "hd": 64}, EUNSUPPORTED, id="pv8: v_scale misaligned is not checked"),
    pytest.param(QK8, {"v_scale": 0x6002, "hd": 72}, EINVAL, id="qk8: v_scale misaligned is"),
    pytest.param("ragged pv8", {"v_scale": 0x6002, "hd": 64}, EINVAL, id="ragged pv8: v_scale misaligned is"),
    pytest.param("window_fp8 pv8", {"v_scale": 0x6002, "hd": 64}, EINVAL, id="window_fp8 pv8: v_scale misaligned is"),
    # the scale vectors and the score bound of another mode are ignored: garbage there does not turn an unsupported call into a malformed one
    pytest.param("ragged bf16", {"k_scale": 0x7002, "v_scale": 0x6002, "hd": 48}, EUNSUPPORTED, id="ragged bf16: scale vectors ignored"),
    pytest.param("ragged pv8", {"k_scale": 0x7002, "hd": 64}, EUNSUPPORTED, id="ragged pv8: k_scale ignored"),
    pytest.param("window_fp8 pv8", {"k_scale": 0x7002, "hd": 64}, EUNSUPPORTED, id="window_fp8 pv8: k_scale ignored"),
    pytest.param("ragged pv8", {"score_bound": -1.0, "hd": 64}, EINVAL, id="ragged pv8: score_bound is checked in every mode"),
    # n_prefix = 0 is a single launch: no workspace, no 16-byte rows
    pytest.param("window", {"n_prefix": 0, "workspace": None, "workspace_bytes": 0, "out": 0x4008, "o_row_stride": 148, "hd": 48}, EUNSUPPORTED,
                 id="window: n_prefix = 0 needs no workspace"),
    pytest.param("window_fp8 pv8", {"n_prefix": 0, "workspace": None, "workspace_bytes": 0, "out": 0x4008, "o_row_stride": 148, "hd": 64},
                 EUNSUPPORTED, id="window_fp8 pv8: n_prefix = 0 needs no workspace"),
]


def _call(entry, changes):
    from open_sora_amd import _C

    assert changes, "the well-formed tuple is never passed: it would launch"
    symbol, _, good = CASES[entry]
    args = {**good, **changes}
    assert list(args) == list(good)
    assert len(args) == len(_C.SIGNATURES[symbol]), symbol
    return getattr(_C.lib, symbol)(*args.values())


@pytest.mark.parametrize("entry, changes, status", SINGLE)
def test_single_fault_status(entry, changes, status):
    assert _call(entry, changes) == status


@pytest.mark.parametrize("entry, changes", DOUBLE)
def test_einval_comes_before_eunsupported(entry, changes):
    assert _call(entry, changes) == EINVAL


@pytest.mark.parametrize("entry, changes, status", DIFFER)
def test_entries_differ_as_recorded(entry, changes, status):
    assert _call(entry, changes) == status


def test_launch_parameters_match_the_recorded_fixture(tmp_path):
    from tools.make_golden_attention_launch_params import OUT, build_probe, run_probe

    with open(OUT) as f:
        gold = json.load(f)
    got = run_probe(build_probe(str(tmp_path)))
    assert got["fields"] == gold["fields"]
    assert [c["call"] for c in got["calls"]] == [c["call"] for c in gold["calls"]]
    bad = []
    for g, w in zip(got["calls"], gold["calls"]):
        if g["status"] != w["status"] or [r[0] for r in g["launches"]] != [r[0] for r in w["launches"]]:
            bad.append((g["call"], "status / launch sequence", (g["status"], [r[0] for r in g["launches"]]), (w["status"], [r[0] for r in w["launches"]])))
            continue
        bad += [(g["call"], f"launch {i} ({rg[0]})", name, a, b) for i, (rg, rw) in enumerate(zip(g["launches"], w["launches"]))
                for name, a, b in zip(gold["fields"], rg, rw) if a != b]
    assert not bad, bad[:8]
    # what the cases are there to show
    kernels = {r[0].split()[0] for c in gold["calls"] for r in c["launches"]}
    assert kernels == {"asm64", "asm72", "asm72w", "asm128", "asm72p8", "asm128p8", "asm128q8", "merge_into"}
    assert all(c["status"] == 0 and c["launches"] for c in gold["calls"])
    col = gold["fields"].index("tail_split")
    assert all(r[col] == 1 for c in gold["calls"] for r in c["launches"]), "no probed launch may carry a tail split: its merge would be a real launch"


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
