"""CPU only: the f64 attention references and derived tolerances of tests/cpu_ops_attn_f64.py hold for a torch emulation of the
kernels on every case of tests/attention_cases.py, and the cases are sensitive enough that five single-key defects of that
emulation leave the tolerance -- before a GPU is involved (tests/test_gpu_attention_audit.py runs the same cases on the device)."""
import pytest
import torch

from tests import attention_cases as A
from tests import cpu_ops_attn_f64 as R

NAMES = [c.name for c in A.CASES]
CLASSES = {"asm72 general", "asm72 FAST", "asm72w FAST", "asm128 general", "asm128 FAST", "asm72p8", "asm128p8", "asm128q8", "auto"}


def _kind(case):
    return "bf16" if case.kind == "bf16" else "fp8"


def _emulate(case, ops, mode, **kw):
    km, vm = kw.pop("km", ops.km), kw.pop("vm", ops.vm)
    parts = case.parts() if case.split > 1 else None
    return R.emulate(ops.qm, km, vm, _kind(case), mode, parts=parts, **kw)


def test_case_table_covers_every_class_and_axis():
    assert {c.klass for c in A.CASES} == CLASSES
    for hd in (64, 72):
        assert any(c.klass == "asm72 FAST" and c.hd == hd for c in A.CASES) and any(c.klass == "asm72w FAST" and c.hd == hd for c in A.CASES)
    assert {1, 37, 63, 64, 65, 128, 129, 192, 300, 321} <= {c.seg for c in A.CASES}
    assert {1, 2, 3, 5} <= {c.n_seg for c in A.CASES}
    assert {1, 31, 33, 255, 256, 257, 300, 1024, 1025, 1100} <= {c.Lq for c in A.CASES}
    for hd in (64, 72, 128):   # every merge instantiation; pv8 and qk8 through the merge
        assert any(c.hd == hd and c.split > 1 and c.api == "bounded" for c in A.CASES)
    assert all(any(c.api == api and c.split > 1 for c in A.CASES) for api in ("pv8", "qk8", "auto"))
    assert any(c.api == "pv8" and c.Bkv and c.prescaled and c.fused for c in A.CASES)
    assert all(c.B <= 2 and c.H <= 3 and c.n_seg * c.seg <= 700 and (c.Lq <= 300 or c.wide) for c in A.CASES)
    for c in A.CASES:
        if c.split > 1:   # a launch smaller than the chip is all tail; whole segments per part, or at least a tile per part
            assert c.units < 128 and (c.n_seg % c.split == 0 if c.n_seg > 1 else c.split <= c.segp // 64), c.name
    assert any(A.operands(c.name).covered for c in A.CASES if c.split > 1 and c.n_seg == 1)
    assert any(A.operands(c.name).covered for c in A.CASES if c.split > 1 and c.n_seg > 1)


@pytest.mark.parametrize("name", NAMES)
def test_selector_rows_lead_by_16_under_the_fast_bound(name):
    c, ops, ref = A.BY_NAME[name], A.operands(name), A.reference(name)
    s, sel = ref["s"], ops.sel
    rows = sel >= 0
    assert rows.any() and (~rows).any()
    if c.n_seg * c.seg > 1:
        picked = s.gather(-1, sel.clamp(min=0)[..., None]).squeeze(-1)
        others = s.scatter(-1, sel.clamp(min=0)[..., None], -1e30).amax(-1)
        lead = (picked - others)[rows].min().item()
        assert lead >= 16.0, lead
    nseg_last = [s_ * c.seg + c.seg - 1 for s_ in range(c.n_seg)]
    if c.B * c.H * c.Lq * 3 // 4 > c.n_seg:
        assert set(nseg_last) <= set(sel[rows].tolist())
    assert sel[0, 0, 0].item() == c.n_seg * c.seg - 1              # the special row: the last valid key
    if c.B * c.H * c.Lq >= 2:
        assert (ops.qm.abs().amax(-1) == 0).sum().item() == 1      # the zero query row
    if c.fast:
        assert ops.bound < 56.0, ops.bound
    if c.api == "auto":   # attn_auto_bound's bound per (batch, head): both sides of the FAST limit in one call
        qn, kn = ops.qm.norm(dim=-1).amax(-1), ops.km.norm(dim=-1).amax(-1)
        b = qn * kn[torch.arange(c.B) % c.nb] * 1.004
        want = torch.tensor([[A.general_pair(c, b_, h) for h in range(c.H)] for b_ in range(c.B)])
        assert ((b > 56.0) == want).all() and want.any() and (~want).any(), b


@pytest.mark.parametrize("name", NAMES)
def test_emulation_stays_inside_the_derived_tolerances(name):
    c, ops, ref = A.BY_NAME[name], A.operands(name), A.reference(name)
    worst = [0.0, 0.0]
    for mode in A.emulation_modes(c, ops):
        for split in ([True, False] if c.api == "auto" and c.split > 1 else [True]):   # the general twin of a pair never splits
            out, lse = _emulate(c, ops, mode) if split else R.emulate(ops.qm, ops.km, ops.vm, _kind(c), mode)
            assert torch.isfinite(out).all() and torch.isfinite(lse).all()
            r = R.ratios(out, lse, ref)
            worst = [max(worst[0], r[0]), max(worst[1], r[1])]
    print(f"emulation {c.klass:15s} {name:40s} err/tol {worst[0]:.3f}  dlse/tol {worst[1]:.3f}")
    assert worst[0] <= 1.0 and worst[1] <= 1.0, worst


def _exceeds(case, ops, ref, mode, **kw):
    out, lse = _emulate(case, ops, mode, **kw)
    r = R.ratios(out, lse, ref)
    return not bool(torch.isfinite(out).all()) or r[0] > 1.0 or r[1] > 1.0


def _mut_drop_last_valid(c, ops):
    if c.seg % 64 == 0:
        return None
    mask = torch.ones(c.n_seg * c.seg)
    mask[c.n_seg * c.seg - 1] = 0.0
    return dict(mask=mask)


def _mut_admit_one_beyond(c, ops):
    if c.seg % 64 == 0:
        return None
    return dict(extra_den=[c.n_seg * c.seg - 1])     # the clamped K row re-fetches the last key: its P once more, against V^T's zero


def _mut_swap_in_tile(c, ops):
    t0 = (c.segp // 64 - 1) * 64
    if c.seg - t0 < 2:
        return None
    i = (c.n_seg - 1) * c.seg + t0
    vm = ops.vm.clone()
    vm[:, :, [i, i + 1]] = ops.vm[:, :, [i + 1, i]]
    return dict(vm=vm)


def _mut_merge_misses_a_part(c, ops):
    return dict(merge_parts=c.split - 1) if c.split > 1 else None


def _mut_v_from_next_segment(c, ops):
    if c.n_seg < 2:
        return None
    vm = ops.vm.clone()
    vm[:, :, c.seg - 1] = ops.vm[:, :, 2 * c.seg - 1]
    return dict(vm=vm)


MUTANTS = {"last_valid_key_of_a_ragged_tile_dropped": _mut_drop_last_valid, "one_key_beyond_seg_len_admitted": _mut_admit_one_beyond,
           "two_keys_swapped_inside_a_vt_tile": _mut_swap_in_tile, "one_key_part_missing_from_the_merge": _mut_merge_misses_a_part,
           "selector_key_v_from_the_next_segment": _mut_v_from_next_segment}


@pytest.mark.parametrize("mutant", list(MUTANTS))
def test_emulation_mutants_leave_the_tolerance(mutant):
    """every mutant is rejected by EVERY case it applies to whose selector rows reach the key it touches -- and by at least one"""
    caught, applicable = [], []
    for c in A.CASES:
        ops = A.operands(c.name)
        kw = MUTANTS[mutant](c, ops)
        if kw is None:
            continue
        applicable.append(c.name)
        if _exceeds(c, ops, A.reference(c.name), A.emulation_modes(c, ops)[0], **kw):
            caught.append(c.name)
    print(f"mutant {mutant}: rejected by {len(caught)} of {len(applicable)} applicable cases; missed by {sorted(set(applicable) - set(caught))}")
    assert caught, applicable
    covered = [n for n in applicable if A.operands(n).covered]
    assert set(covered) <= set(caught), sorted(set(covered) - set(caught))
