#!/usr/bin/env python
"""What the qk8 attention costs ONE sequence-parallel rank per block against the pv8 attention, at the rank shape of BASELINE
configs[4] (11B, head_dim 128, 24 heads, B = 1, L = 230,912 = 8 segments of 28,864 keys), on ONE GPU, no collectives:
`python tools/sp_qk8_time.py [--quick]` prints one JSON line (recorded in profiles/attn_qk8_sp.md).

Each arm is everything seqpar.SeqPar launches on the compute stream for the exchange and the attention of one block in all-gather mode:

    pv8   osk_v_scale_fp8(v)        + osk_copy_rows_bf16(k -> gather slot) + osk_v_transpose_fp8 + osk_attention_fwd_pv8_bf16
    qk8   osk_kv_scale_fp8(k, v)    + osk_k_pack_fp8(k -> gather slot)     + osk_v_transpose_fp8 + osk_attention_fwd_qk8_bf16

over this rank's 28,864 rows for the first three and the 8 gathered segments for the launch (the other 7 segments are packed once,
outside the timing: their ranks do that).  The two arms ALTERNATE round by round (tools/rank_shapes.py::attention_qk8_ab), per arm
the median of the rounds' medians and the rounds' spread.  The pieces the qk8 arm adds or replaces are also timed alone, with the
bytes osk_kv_scale_fp8 reads per second.  The figure to hold the ratio against is the single-device one of profiles/attn_qk8.md."""
from __future__ import annotations

import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from tools.rank_shapes import BF, LOG2E, QK8_SHAPES, _events, _unit_rms

SINGLE_DEVICE_RATIO = {"source": "profiles/attn_qk8.md, configs[4] rank row", "pv8_ms": 52.092, "qk8_ms": 39.828, "k_scale_pack_ms": 0.674,
                       "qk8_plus_pack_vs_pv8": 0.778}


def measure(dev, rounds=5, iters=3, warm=2) -> dict:
    from open_sora_amd import _C

    B, H, Lloc, P, _ = QK8_SHAPES["cfg4_rank"]
    hd, D, rank = 128, H * 128, 3
    g = torch.Generator(device=dev).manual_seed(5)
    q = (_unit_rms(torch.randn(B, Lloc, D, device=dev, generator=g), H, hd) * (hd ** -0.5 * LOG2E)).to(BF)
    k = _unit_rms(torch.randn(P, B, Lloc, D, device=dev, generator=g), H, hd).to(BF)
    v = torch.randn(P, B, Lloc, D, device=dev, generator=g).to(BF)
    segp = (Lloc + 63) // 64 * 64
    ws = _C.attention_workspace(q.device)
    # what the ranks hold after the reduction: the scales of the WHOLE sequence, both vectors in one [2, B, H] buffer
    s2 = _C.kv_scale_fp8(k.view(P * B, Lloc, D), v.view(P * B, Lloc, D), H, hd).view(2, P, B, H).amax(1).contiguous()
    k_all = torch.empty(P, B, Lloc, D, dtype=BF, device=dev)
    k_all.copy_(k)
    k8_all = torch.empty(P, *_C.k8_shape(B, H, Lloc), dtype=torch.uint8, device=dev)
    vt8_all = torch.zeros(P, B, H, _C.vt8_rows(hd), segp, dtype=torch.uint8, device=dev)
    for s_ in range(P):
        _C.k_pack_fp8(k[s_], s2[0], k8_all[s_], H, hd)
        _C.v_transpose_fp8(v[s_], s2[1], vt8_all[s_], H, hd)
    kl, vl = k[rank], v[rank]
    loc2 = torch.empty(2, B, H, dtype=torch.float32, device=dev)          # this rank's own (unreduced) scales: computed, not used
    outs = {n: torch.empty(B, Lloc, D, dtype=BF, device=dev) for n in ("pv8", "qk8")}

    def arm_pv8():
        _C.v_scale_fp8(vl, H, hd)
        _C.copy_rows(kl, k_all[rank])
        _C.v_transpose_fp8(vl, s2[1], vt8_all[rank], H, hd)
        _C.attention_fwd_pv8(q, k_all[0], vt8_all, s2[1], outs["pv8"], H, hd, hd ** -0.5, n_seg=P, seg_len=Lloc,
                             k_seg_stride=k_all.stride(0), vt_seg_stride=vt8_all.stride(0), q_prescaled=True, workspace=ws)

    def arm_qk8():
        _C.kv_scale_fp8(kl, vl, H, hd, out=loc2)
        _C.k_pack_fp8(kl, s2[0], k8_all[rank], H, hd)
        _C.v_transpose_fp8(vl, s2[1], vt8_all[rank], H, hd)
        _C.attention_fwd_qk8(q, k8_all[0], s2[0], vt8_all, s2[1], outs["qk8"], H, hd, hd ** -0.5, seg_len=Lloc, n_seg=P,
                             k_seg_stride=k8_all.stride(0), vt_seg_stride=vt8_all.stride(0), q_prescaled=True, workspace=ws)

    fns = {"pv8": arm_pv8, "qk8": arm_qk8}
    ms = {n: [] for n in fns}
    for r in range(rounds):
        for n in (("pv8", "qk8") if r % 2 == 0 else ("qk8", "pv8")):
            ms[n].append(_events(fns[n], iters, warm))
    assert all(torch.isfinite(o.float()).all() for o in outs.values())
    assert torch.equal(loc2, torch.stack([_C.v_scale_fp8(kl, H, hd), _C.v_scale_fp8(vl, H, hd)]))
    med = lambda x: sorted(x)[len(x) // 2]
    pieces = {"kv_scale_fp8": lambda: _C.kv_scale_fp8(kl, vl, H, hd, out=loc2), "v_scale_fp8": lambda: _C.v_scale_fp8(vl, H, hd),
              "k_pack_fp8": lambda: _C.k_pack_fp8(kl, s2[0], k8_all[rank], H, hd), "copy_rows_k": lambda: _C.copy_rows(kl, k_all[rank]),
              "v_transpose_fp8": lambda: _C.v_transpose_fp8(vl, s2[1], vt8_all[rank], H, hd)}
    t = {n: _events(f, 9, 3) for n, f in pieces.items()}
    rel = ((outs["qk8"].double() - outs["pv8"].double()).norm() / outs["pv8"].double().norm()).item()
    res = {"device": torch.cuda.get_device_name(dev), "shape": {"B": B, "H": H, "hd": hd, "rows_per_rank": Lloc, "n_seg": P, "keys": P * Lloc},
           "timing": f"{rounds} rounds, arms alternating, {warm} warm-up + {iters} timed runs of the whole arm per round (device events, median)"}
    for n in fns:
        m = med(ms[n])
        res[n] = {"ms_per_block": round(m, 3), "rounds_ms": [round(x, 3) for x in ms[n]], "spread": round((max(ms[n]) - min(ms[n])) / m, 4)}
    res["pieces_ms"] = {n: round(x, 4) for n, x in t.items()}
    kv_bytes = 2.0 * B * Lloc * D * 2
    res["kv_scale_fp8"] = {"bytes_read": kv_bytes, "workgroups": 2 * B * H, "tb_per_s": round(kv_bytes / t["kv_scale_fp8"] / 1e9, 3)}
    res["qk8_vs_pv8"] = round(res["qk8"]["ms_per_block"] / res["pv8"]["ms_per_block"], 4)
    res["single_device"] = SINGLE_DEVICE_RATIO
    res["rel_l2_qk8_vs_pv8"] = round(rel, 5)
    return res


if __name__ == "__main__":
    quick = "--quick" in sys.argv[1:]
    print(json.dumps(measure(torch.device("cuda", 0), rounds=3 if quick else 5)), flush=True)
