"""Time one sequence-parallel rank's attention per block with and without frame-window attention, on ONE GPU, at the long shape
(512 text + 51 x 3,600 image tokens = 184,112 rows) split for P = 8 (23,014 rows per rank), XL head geometry (H 16, head_dim 72):

  allgather  the rank's 23,014 queries against all keys, 16 heads
             (a) today's call: osk_attention_fwd_bounded_bf16 over 8 key segments (seqpar.SeqPar.attention)
             (b) osk_kv_join_bf16 + ONE osk_attention_fwd_window_bf16 with the table of the rank's rows
  ulysses    the 8 received query chunks against all keys, the rank's H / P = 2 heads
             (a) today's calls: osk_v_transpose_bf16 of the received V + the one launch over 8 segments and 8 B query batches
             (b) osk_kv_join_bf16 + EIGHT window calls, one per source rank with that rank's table

B = 1 and B = 3, W = 2 and 8.  Also timed alone: the join, and osk_v_transpose_bf16 on a contiguous V of the same size, each with
its achieved HBM bandwidth (the join moves 4 x B x L x D x 2 bytes, the transpose half of that).  Every arm of a (mode, B) is warmed
up, then the arms alternate in one process: `repeats` rounds, each call between two device events.  The exchange itself (the
collectives, and what of them the window leaves exposed) needs a multi-GPU node and is NOT measured here.  No threshold is set.

    python tools/sp_window_time.py [--repeats 5] [--rank 3] [--out profiles/sp_window_time.jsonl]

--fp8 pv8|qk8: the same comparison in fp8 mode at the 11B head geometry (H 24, head_dim 128; main_fp8): the unwindowed
segment-addressed fp8 call against osk_kv_quant_rows_fp8 + osk_kv_join_fp8 + the fp8 window call(s), the two new kernels alone with
their GB/s, and the bytes a rank gathers per block before / after.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.attn_window_time import time_arms  # noqa: E402

P, H, HD, L_TXT, N, T = 8, 16, 72, 512, 3600, 51
WINDOWS = (2, 8)
BF = torch.bfloat16


def _emitter(a):
    def emit(row):
        print(json.dumps(row), flush=True)
        if a.out:
            path = a.out if os.path.isabs(a.out) else os.path.join(ROOT, a.out)
            os.makedirs(os.path.dirname(path), exist_ok=True)
            with open(path, "a") as f:
                f.write(json.dumps(row) + "\n")

    return emit


H8, HD8 = 24, 128     # the 11B model's heads (BASELINE configs[4]); head exchange: H / P = 3 heads per rank


def main_fp8(a, _C, mmdit, dev):
    """--fp8 pv8 | qk8: one rank's cost per block in fp8 mode at the 11B head geometry, the same sequence and split.
      allgather  full: the unwindowed segment-addressed fp8 call over 8 key segments (seqpar.SeqPar.attention)
                 window: osk_kv_quant_rows_fp8 of the rank's own rows (V; K too under qk8) + osk_kv_join_fp8 + ONE fp8 window call
      ulysses    full: the packs of the received chunks (osk_v_transpose_fp8; osk_k_pack_fp8 under qk8) + the one launch
                 window: osk_kv_quant_rows_fp8 of the received chunks + osk_kv_join_fp8 + EIGHT window calls
    The scale launches are the same on both sides and are left out of both.  Also timed alone: the quantisation and the join with
    their achieved HBM bandwidth, and (all-gather mode) the rank's own packs of the unwindowed path.  One more row per (mode, B) states
    the bytes a rank receives per block, before (bf16 window path; unwindowed fp8 exchange) and after."""
    fmode, qk8 = a.fp8, a.fp8 == "qk8"
    emit = _emitter(a)
    U8 = torch.uint8
    L = L_TXT + N * T
    Lc = -(-L // P)
    Ltail = L - (P - 1) * Lc
    rows_of = lambda r: Ltail if r == P - 1 else Lc
    RP = _C.vt8_rows(HD8)
    Lcp, Lp = (Lc + 63) // 64 * 64, (L + 63) // 64 * 64
    for B in (int(x) for x in a.batches.split(",")):
        for mode in ("allgather", "ulysses"):
            Hl = H8 if mode == "allgather" else H8 // P
            D = Hl * HD8
            g = torch.Generator(device=dev).manual_seed(7)
            k_seg = torch.randn(P, B, Lc, D, device=dev, generator=g).to(BF)
            v_seg = torch.randn(P, B, Lc, D, device=dev, generator=g).to(BF)
            k_seg[P - 1][:, Ltail:] = 0          # the zero pad rows of a ragged split's last chunk
            v_seg[P - 1][:, Ltail:] = 0
            kn = float(k_seg.float().view(P, B, Lc, Hl, HD8).norm(dim=-1).max())
            nq = 1 if mode == "allgather" else P
            q = torch.randn(nq, B, Lc, D, device=dev, generator=g)
            q = (q * (40.0 / (float(q.view(nq, B, Lc, Hl, HD8).norm(dim=-1).max()) * kn))).to(BF)
            out = torch.empty_like(q)
            k3, v3 = k_seg.view(P * B, Lc, D), v_seg.view(P * B, Lc, D)
            s2 = _C.kv_scale_fp8(k3, v3, Hl, HD8).view(2, P, B, Hl).amax(1).contiguous()         # [2, B, Hl]
            s2p = s2.repeat(1, P, 1).contiguous()                                               # [2, P * B, Hl]
            # the unwindowed path's operands: e4m3 V^T (and K under qk8) per segment
            vt8_seg = torch.zeros(P, B, Hl, RP, Lcp, dtype=U8, device=dev)
            k8_seg = torch.empty(P, *_C.k8_shape(B, Hl, Lc, HD8), dtype=U8, device=dev) if qk8 else None

            def packs():
                _C.v_transpose_fp8(v3, s2p[1], vt8_seg.view(P * B, Hl, RP, Lcp), Hl, HD8)
                if qk8:
                    _C.k_pack_fp8(k3, s2p[0], k8_seg.view(P * B, Hl, Lcp, 128), Hl, HD8)

            r0 = a.rank
            own_vt8 = torch.empty(B, Hl, RP, Lcp, dtype=U8, device=dev)
            own_k8 = torch.empty(_C.k8_shape(B, Hl, Lc, HD8), dtype=U8, device=dev) if qk8 else None

            def pack_own():
                _C.v_transpose_fp8(v_seg[r0], s2[1], own_vt8, Hl, HD8)
                if qk8:
                    _C.k_pack_fp8(k_seg[r0], s2[0], own_k8, Hl, HD8)

            packs()
            ws_full = _C.attention_workspace(dev)

            def full_call():
                qq, oo = q.view(nq * B, Lc, D), out.view(nq * B, Lc, D)
                kvb = B if mode == "ulysses" else 0
                if qk8:
                    _C.attention_fwd_qk8(qq, k8_seg[0], s2[0], vt8_seg, s2[1], oo, Hl, HD8, HD8 ** -0.5, seg_len=Lc, n_seg=P,
                                         k_seg_stride=k8_seg.stride(0), vt_seg_stride=vt8_seg.stride(0), q_prescaled=True, kv_batches=kvb, workspace=ws_full)
                else:
                    _C.attention_fwd_pv8(qq, k_seg[0], vt8_seg, s2[1], oo, Hl, HD8, HD8 ** -0.5, n_seg=P, seg_len=Lc, k_seg_stride=k_seg.stride(0),
                                         vt_seg_stride=vt8_seg.stride(0), q_prescaled=True, kv_batches=kvb, workspace=ws_full)

            full = full_call if mode == "allgather" else (lambda: (packs(), full_call()))
            # the window path: token-major e4m3 segments, the joined operands
            v8 = torch.empty(P, B, Lc, D, dtype=U8, device=dev)
            k8t = torch.empty(P, B, Lc, D, dtype=U8, device=dev) if qk8 else None
            kj = torch.empty(_C.k8_shape(B, Hl, L, HD8), dtype=U8, device=dev) if qk8 else torch.empty(B, L, D, dtype=BF, device=dev)
            vtj = torch.empty(B, Hl, RP, Lp, dtype=U8, device=dev)
            ws_win = torch.empty(_C.attention_window_workspace_bytes(B, Hl, Lc, HD8), dtype=U8, device=dev)

            def quant_all():
                _C.kv_quant_rows_fp8(v3, s2p[1], v8.view(P * B, Lc, D), Hl, HD8)
                if qk8:
                    _C.kv_quant_rows_fp8(k3, s2p[0], k8t.view(P * B, Lc, D), Hl, HD8)

            def quant_own():
                _C.kv_quant_rows_fp8(v_seg[r0], s2[1], v8[r0], Hl, HD8)
                if qk8:
                    _C.kv_quant_rows_fp8(k_seg[r0], s2[0], k8t[r0], Hl, HD8)

            quant_all()
            quant = quant_own if mode == "allgather" else quant_all
            join = lambda: _C.kv_join_fp8(k8t if qk8 else k_seg, v8, kj, vtj, Hl, HD8, L)
            ranks = [a.rank] if mode == "allgather" else list(range(P))
            tables = {w: [mmdit.attention_window_table(L_TXT, N * T, N, w, row0=r * Lc, n_rows=rows_of(r)) for r in ranks] for w in WINDOWS}

            def window_calls(w):
                for i, t in enumerate(tables[w]):
                    rows = rows_of(ranks[i])
                    _C.attention_fwd_window_fp8(q[i][:, :rows], kj, s2[0] if qk8 else None, vtj, s2[1], out[i][:, :rows], Hl, HD8, HD8 ** -0.5,
                                                n_prefix=L_TXT, windows=t, mode=fmode, q_prescaled=True, workspace=ws_win, Lk=L)

            arms = {"full": full, "quant": quant, "join": join}
            if mode == "allgather":
                arms["pack_own"] = pack_own
            for w in WINDOWS:
                arms[f"W{w}_calls"] = lambda w=w: window_calls(w)
                arms[f"W{w}_quant+join+calls"] = lambda w=w: (quant(), join(), window_calls(w))
            ms = time_arms(arms, a.warmup, a.repeats, 1)
            med = {n_: statistics.median(x) for n_, x in ms.items()}
            n_q = (B if mode == "allgather" else P * B) * Lc * D * (2 if qk8 else 1)           # elements quantised
            join_bytes = B * L * D + B * Hl * RP * Lp + (B * L * D + B * Hl * Lp * 128 if qk8 else 4 * B * L * D)
            for n_ in arms:
                row = dict(what="sp_window_time_fp8", fp8=fmode, mode=mode, P=P, rank=a.rank if mode == "allgather" else "all source ranks", B=B,
                           heads=Hl, hd=HD8, L=L, rows_per_rank=Lc, last_rank_rows=Ltail, arm=n_, repeats=a.repeats, ms=[round(x, 4) for x in ms[n_]],
                           median_ms=round(med[n_], 4), spread_ms=round(max(ms[n_]) - min(ms[n_]), 4))
                if n_ == "quant":
                    row["bytes"] = 3 * n_q                       # 2 bytes read, 1 written per element
                    row["GBps"] = round(row["bytes"] / med[n_] * 1e-6, 1)
                elif n_ == "join":
                    row["bytes"] = join_bytes
                    row["GBps"] = round(row["bytes"] / med[n_] * 1e-6, 1)
                elif n_.startswith("W"):
                    w = int(n_[1:].split("_")[0])
                    fr = [mmdit.window_tile_fraction(t, L_TXT, N * T) * t.shape[0] for t in tables[w]]
                    row["window_frames"] = w
                    row["tile_fraction"] = round(sum(fr) / sum(t.shape[0] for t in tables[w]), 4)
                    row["window_launches"] = len(tables[w])
                    row["time_ratio_to_full"] = round(med[n_] / med["full"], 4)
                    if n_.endswith("join+calls"):
                        row["quant_share"] = round(med["quant"] / med[n_], 4)
                        row["join_share"] = round(med["join"] / med[n_], 4)
                emit(row)
            if mode == "allgather":
                # bytes a rank's gather buffers hold per block (P slots; (P - 1) / P of them arrive over the links)
                tok = P * B * Lc * H8 * HD8
                emit(dict(what="sp_window_exchange_bytes", fp8=fmode, mode=mode, P=P, B=B, gathered_bytes_bf16_window=4 * tok,
                          gathered_bytes_fp8_unwindowed=P * B * H8 * RP * Lcp + (P * B * H8 * Lcp * 128 if qk8 else 2 * tok),
                          gathered_bytes_fp8_window=tok + (tok if qk8 else 2 * tok), measured=False))
            del q, out, k_seg, v_seg, vt8_seg, k8_seg, v8, k8t, kj, vtj, ws_win, own_vt8, own_k8, k3, v3
            torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--rank", type=int, default=3, help="the all-gather arm's rank (a middle rank: no text rows)")
    ap.add_argument("--batches", default="1,3")
    ap.add_argument("--out", default=None)
    ap.add_argument("--fp8", choices=("pv8", "qk8"), default=None, help="the fp8 arm at the 11B head geometry (H 24, head_dim 128)")
    a = ap.parse_args()
    assert a.repeats >= 3, "at least 3 rounds of every arm"

    from open_sora_amd import _C, mmdit

    dev = "cuda:0"
    torch.cuda.set_device(0)
    if a.fp8:
        return main_fp8(a, _C, mmdit, dev)
    L = L_TXT + N * T
    Lc = -(-L // P)
    Ltail = L - (P - 1) * Lc
    rows_of = lambda r: Ltail if r == P - 1 else Lc

    emit = _emitter(a)
    for B in (int(x) for x in a.batches.split(",")):
        for mode in ("allgather", "ulysses"):
            Hl = H if mode == "allgather" else H // P
            D = Hl * HD
            g = torch.Generator(device=dev).manual_seed(7)
            Lcp, Lp = (Lc + 63) // 64 * 64, (L + 63) // 64 * 64
            # the gathered buffers as seqpar.py holds them: K and V token-major [P, B, Lc, D]; V^T per segment for today's call
            k_seg = torch.randn(P, B, Lc, D, device=dev, generator=g).to(BF)
            v_seg = torch.randn(P, B, Lc, D, device=dev, generator=g).to(BF)
            kn = float(k_seg.float().view(P, B, Lc, Hl, HD).norm(dim=-1).max())
            nq = 1 if mode == "allgather" else P             # query chunks in hand: this rank's, or one per source rank
            q = torch.randn(nq, B, Lc, D, device=dev, generator=g)
            q = (q * (40.0 / (float(q.view(nq, B, Lc, Hl, HD).norm(dim=-1).max()) * kn))).to(BF)   # prescaled, |q||k| <= ~40 < 56
            bound = float(q.float().view(nq, B, Lc, Hl, HD).norm(dim=-1).max()) * kn * 1.01
            out = torch.empty_like(q)
            vt_seg = torch.zeros(P, B, Hl, HD, Lcp, dtype=BF, device=dev)
            kj = torch.empty(B, L, D, dtype=BF, device=dev)
            vtj = torch.empty(B, Hl, HD, Lp, dtype=BF, device=dev)
            v_flat = torch.randn(B, L, D, device=dev, generator=g).to(BF)      # a contiguous V of the same size, for the transpose alone
            vt_flat = torch.empty(B, Hl, HD, Lp, dtype=BF, device=dev)
            ws_full = _C.attention_workspace(dev)
            ws_win = torch.empty(_C.attention_window_workspace_bytes(B, Hl, Lc, HD), dtype=torch.uint8, device=dev)

            def transpose_segments():
                _C.v_transpose(v_seg.view(P * B, Lc, D), vt_seg.view(P * B, Hl, HD, Lcp), Hl, HD)

            transpose_segments()
            join = lambda: _C.kv_join(k_seg, v_seg, kj, vtj, Hl, HD, L)

            def full():
                if mode == "ulysses":
                    transpose_segments()
                _C.attention_fwd(q.view(nq * B, Lc, D), k_seg[0], vt_seg, out.view(nq * B, Lc, D), Hl, HD, HD ** -0.5, n_seg=P, seg_len=Lc,
                                 k_seg_stride=k_seg.stride(0), vt_seg_stride=vt_seg.stride(0), q_prescaled=True,
                                 kv_batches=B if mode == "ulysses" else 0, workspace=ws_full, score_bound=bound)

            ranks = [a.rank] if mode == "allgather" else list(range(P))
            tables = {w: [mmdit.attention_window_table(L_TXT, N * T, N, w, row0=r * Lc, n_rows=rows_of(r)) for r in ranks] for w in WINDOWS}

            def window_calls(w):
                for i, t in enumerate(tables[w]):
                    rows = rows_of(ranks[i])
                    _C.attention_fwd_window(q[i][:, :rows], kj, vtj, out[i][:, :rows], Hl, HD, HD ** -0.5, n_prefix=L_TXT, windows=t,
                                            q_prescaled=True, score_bound=bound, workspace=ws_win)

            arms = {"full": full, "join": join, "v_transpose_contiguous": lambda: _C.v_transpose(v_flat, vt_flat, Hl, HD)}
            for w in WINDOWS:
                arms[f"W{w}_calls"] = lambda w=w: window_calls(w)
                arms[f"W{w}_join+calls"] = lambda w=w: (join(), window_calls(w))
            ms = time_arms(arms, a.warmup, a.repeats, 1)
            med = {n_: statistics.median(x) for n_, x in ms.items()}
            for n_ in arms:
                row = dict(what="sp_window_time", mode=mode, P=P, rank=a.rank if mode == "allgather" else "all source ranks", B=B, heads=Hl,
                           hd=HD, L=L, rows_per_rank=Lc, last_rank_rows=Ltail, arm=n_, repeats=a.repeats, ms=[round(x, 4) for x in ms[n_]],
                           median_ms=round(med[n_], 4), spread_ms=round(max(ms[n_]) - min(ms[n_]), 4), score_bound=round(bound, 3))
                if n_ == "join":
                    row["bytes"] = 4 * B * L * D * 2
                    row["GBps"] = round(row["bytes"] / med[n_] * 1e-6, 1)
                elif n_ == "v_transpose_contiguous":
                    row["bytes"] = 2 * B * L * D * 2
                    row["GBps"] = round(row["bytes"] / med[n_] * 1e-6, 1)
                elif n_ != "full":
                    w = int(n_[1:].split("_")[0])
                    # key tiles the calls visit / those the full call does, over the query blocks in hand (text tiles included)
                    fr = [mmdit.window_tile_fraction(t, L_TXT, N * T) * t.shape[0] for t in tables[w]]
                    row["window_frames"] = w
                    row["tile_fraction"] = round(sum(fr) / sum(t.shape[0] for t in tables[w]), 4)
                    row["window_launches"] = len(tables[w])
                    row["time_ratio_to_full"] = round(med[n_] / med["full"], 4)
                    if n_.endswith("join+calls"):
                        row["join_share"] = round(med["join"] / med[n_], 4)
                emit(row)
            del q, out, k_seg, v_seg, vt_seg, kj, vtj, v_flat, vt_flat, ws_win
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
