#!/usr/bin/env python
"""What the chunked K / V^T gather (seqpar.enable(..., kv_chunks=S)) COSTS one sequence-parallel rank per block, on ONE GPU, no
collectives: `python tools/sp_chunk_time.py [--quick] [--write]` prints one JSON line and, with --write, rewrites the table of
profiles/sp_chunked.md between its markers (`--from-json FILE` renders a recorded line, without a GPU).

Rank shapes of BASELINE configs[3] (XL, 16 x 72, 8 x 23,014 keys) and configs[4] (11B, 24 x 128, 8 x 28,864 keys), all-gather
mode, bf16 attention.  Per S in {1, 2, 4, 8} (the effective count for the rank's rows: the largest S' <= S dividing them) one arm =
everything seqpar.SeqPar launches on the compute stream for the exchange and the attention of one block:

    S = 1   osk_copy_rows_bf16(k -> gather slot) + osk_v_transpose_bf16(v -> gather slot) + ONE osk_attention_fwd_bounded_bf16
            over 8 segments of L/P keys
    S > 1   S x (copy + transpose of a slice) + S launches over 8 segments of L/(P S) keys, each with lse, + osk_attention_merge_bf16

The other ranks' slots are filled once, outside the timing.  The arms alternate round by round; per arm the median of the rounds'
medians and the rounds' spread.  The merge is also timed alone (HBM bytes per second).

THIS IS THE COST SIDE ONLY: launch granularity (S shorter key loops per work unit, S grid tails) plus the merge.  What the slices
buy -- attention on slice 0 while slices 1 .. S-1 travel -- needs ranks that exchange over xGMI, i.e. a multi-GPU node."""
from __future__ import annotations

import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from tools.rank_shapes import BF, LOG2E, SHAPES, _events, _unit_rms

MARK0, MARK1 = "<!-- sp_chunk_time:begin -->", "<!-- sp_chunk_time:end -->"


def effective(S: int, Lloc: int) -> int:
    return max(s for s in range(1, S + 1) if Lloc % s == 0)


def measure_shape(dev, name, rounds=3, iters=2, warm=1) -> dict:
    from open_sora_amd import _C

    _, D, H, hd, P, Lloc, B = SHAPES[name]
    rank = 3
    g = torch.Generator(device=dev).manual_seed(5)
    q = (_unit_rms(torch.randn(B, Lloc, D, device=dev, generator=g), H, hd) * (hd ** -0.5 * LOG2E)).to(BF)
    k = _unit_rms(torch.randn(P, B, Lloc, D, device=dev, generator=g), H, hd).to(BF)
    v = torch.randn(P, B, Lloc, D, device=dev, generator=g).to(BF)
    qn = q.float().view(B, Lloc, H, hd).norm(dim=-1).amax().item()
    kn = k.float().view(P, B, Lloc, H, hd).norm(dim=-1).amax().item()
    bound = 1.02 * qn * kn                         # what mmdit._score_bound derives from unit QK-norm scales, on the data
    ws = _C.attention_workspace(q.device)
    out = {}
    arms, bufs = {}, {}
    for S in sorted({effective(S, Lloc) for S in (1, 2, 4, 8)}):
        Lc = Lloc // S
        Lcp = (Lc + 63) // 64 * 64
        k_all = torch.empty(S, P, B, Lc, D, dtype=BF, device=dev)
        vt_all = torch.zeros(S, P, B, H, hd, Lcp, dtype=BF, device=dev)
        for s in range(S):
            for r in range(P):
                k_all[s, r].copy_(k[r][:, s * Lc:(s + 1) * Lc])
                _C.v_transpose(v[r][:, s * Lc:(s + 1) * Lc], vt_all[s, r], H, hd)
        o = torch.empty(B, Lloc, D, dtype=BF, device=dev)
        parts = torch.empty(S, B, Lloc, D, dtype=BF, device=dev) if S > 1 else None
        lses = torch.empty(S, B, H, Lloc, dtype=torch.float32, device=dev) if S > 1 else None
        bufs[S] = (k_all, vt_all, o, parts, lses)

        def arm(S=S, Lc=Lc, k_all=k_all, vt_all=vt_all, o=o, parts=parts, lses=lses):
            for s in range(S):
                _C.copy_rows(k[rank][:, s * Lc:(s + 1) * Lc], k_all[s, rank])
                _C.v_transpose(v[rank][:, s * Lc:(s + 1) * Lc], vt_all[s, rank], H, hd)
            for s in range(S):
                _C.attention_fwd(q, k_all[s, 0], vt_all[s], o if S == 1 else parts[s], H, hd, hd ** -0.5,
                                 lse=None if S == 1 else lses[s], n_seg=P, seg_len=Lc, k_seg_stride=k_all.stride(1),
                                 vt_seg_stride=vt_all.stride(1), q_prescaled=True, workspace=ws, score_bound=bound)
            if S > 1:
                _C.attention_merge(parts, lses, o, H, hd)

        arms[S] = arm
    ms = {S: [] for S in arms}
    order = list(arms)
    for r in range(rounds):
        for S in (order if r % 2 == 0 else order[::-1]):
            ms[S].append(_events(arms[S], iters, warm))
    med = lambda x: sorted(x)[len(x) // 2]
    ref = bufs[1][2].double()
    base = med(ms[1])
    res = {"shape": {"B": B, "H": H, "hd": hd, "rows_per_rank": Lloc, "n_seg": P, "keys": P * Lloc}, "score_bound": round(bound, 2),
           "timing": f"{rounds} rounds, arms alternating, {warm} warm-up + {iters} timed runs of the whole arm per round (device events, median)",
           "arms": {}}
    for S in order:
        k_all, vt_all, o, parts, lses = bufs[S]
        assert torch.isfinite(o.float()).all()
        m = med(ms[S])
        rec = {"asked_for": [a for a in (1, 2, 4, 8) if effective(a, Lloc) == S], "keys_per_slice_segment": Lloc // S,
               "body": _C.attention_body(hd, P, Lloc // S, bound), "ms_per_block": round(m, 3), "rounds_ms": [round(x, 3) for x in ms[S]],
               "spread": round((max(ms[S]) - min(ms[S])) / m, 4), "vs_one_gather": round(m / base, 4)}
        if S > 1:
            t = _events(lambda: _C.attention_merge(parts, lses, o, H, hd), 9, 3)
            nbytes = (S + 1) * B * Lloc * D * 2 + S * B * H * Lloc * 4
            rec["merge_ms"] = round(t, 4)
            rec["merge_tb_per_s"] = round(nbytes / t / 1e9, 3)
            rec["partials_mb"] = round((parts.numel() * 2 + lses.numel() * 4) / 2 ** 20, 1)
            rec["rel_l2_vs_one_gather"] = float(f"{((o.double() - ref).norm() / ref.norm()).item():.3e}")
        res["arms"][str(S)] = rec
    return res


def table(res: dict) -> str:
    lines = ["| rank shape | S (asked for) | keys per slice segment | loop body | ms per block | vs S = 1 | rounds' spread | merge ms | merge TB/s | relL2 vs S = 1 |",
             "|---|---|---|---|---|---|---|---|---|---|"]
    for name, rec in res["shapes"].items():
        sh = rec["shape"]
        for S, a in rec["arms"].items():
            lines.append(f"| {name}: {sh['H']} x {sh['hd']}, {sh['rows_per_rank']} rows, {sh['keys']} keys | {S} ({', '.join(map(str, a['asked_for']))}) | "
                         f"{a['keys_per_slice_segment']} | {a['body']} | {a['ms_per_block']} | {a['vs_one_gather']} | {a['spread']} | "
                         f"{a.get('merge_ms', '-')} | {a.get('merge_tb_per_s', '-')} | {a.get('rel_l2_vs_one_gather', '-')} |")
    return "\n".join(lines)


def write_profile(res: dict, path: str) -> None:
    text = open(path).read()
    a, b = text.index(MARK0) + len(MARK0), text.index(MARK1)
    body = f"\n{res['device']}; {res['shapes']['cfg3']['timing']}.\n\n{table(res)}\n"
    with open(path, "w") as f:
        f.write(text[:a] + body + text[b:])


if __name__ == "__main__":
    if "--from-json" in sys.argv[1:]:             # render a recorded JSON line into the profile (no GPU needed)
        with open(sys.argv[sys.argv.index("--from-json") + 1]) as f:
            write_profile(json.loads(f.read().strip().splitlines()[-1]), os.path.join(ROOT, "profiles", "sp_chunked.md"))
        sys.exit(0)
    quick = "--quick" in sys.argv[1:]
    dev = torch.device("cuda", 0)
    res = {"device": torch.cuda.get_device_name(dev), "what": "cost side of the chunked gather on one GPU: S launches + the merge against one launch",
           "shapes": {}}
    for name in ("cfg3", "cfg4"):
        res["shapes"][name] = measure_shape(dev, name, rounds=3 if quick else 5)
        torch.cuda.empty_cache()
    print(json.dumps(res), flush=True)
    if "--write" in sys.argv[1:]:
        write_profile(res, os.path.join(ROOT, "profiles", "sp_chunked.md"))
