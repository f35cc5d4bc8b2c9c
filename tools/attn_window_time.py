"""Time osk_attention_fwd_window_bf16 (frame-window attention: text prefix + one run of image key tiles per 256-row query block)
against full attention, at the kernel level, on two shapes:

  headline   B = 3, H = 16, head_dim 72, 512 text + 16 x 1,024 image tokens (bench.py's step), W in {1, 2, 4, 16}
  long       B = 1, H = 16, head_dim 72, 512 text + 51 x 3,600 image tokens (BASELINE configs[3]),  W in {2, 8}

The baseline arm is the call the model makes without a window: osk_attention_fwd_bounded_bf16 with the tail-split workspace
(_C.attention_fwd).  Both arms get the same q, k, V^T and the same score bound (the FAST body).  Per shape, ONE process: every arm
is warmed up, then the arms alternate, `repeats` rounds of `inner` back-to-back calls each between two device events.  Printed per
arm: the median time, the spread, the visited-tile fraction (text tiles included, mmdit.window_tile_fraction), the time ratio to the
baseline and that ratio over the tile fraction (1.0 = time follows the tiles).  W = 16 at the headline shape has every range full:
it prices the second launch, the merge and the loss of the wide layout and of the tail split.  No threshold is set.

--mode pv8 | qk8: the fp8 entry, osk_attention_fwd_window_fp8_bf16, at the 11B head geometry (H = 24, head_dim 128): 512 + 16 x 1,024
tokens at B = 3 and the long shape at B = 1, W in {1, 2, 4} and every range full.  The baseline arm is the full fp8 call of the SAME
mode (osk_attention_fwd_pv8_bf16 / osk_attention_fwd_qk8_bf16 with the tail-split workspace); every arm is timed twice, the launch
alone on prepared operands and ("+pack") with the scale kernels, the V^T pack and in qk8 mode the K pack in front of it, which
touch every key whatever the window.

--anchors h,t (bf16 mode): anchor frames (osk_attention_fwd_window_anchor_bf16).  Per shape, at W in {1, 2} (headline) / {2} (long),
three alternating arms -- the full call, the un-anchored window call of that W, the anchored call -- and, on the same rows, the
one-pass three-part merge (osk_attention_merge_into2_bf16) against two passes of osk_attention_merge_into_bf16.  The anchored arm's
ratios are printed against both other arms.  No threshold is set; output quality is not measured.

    python tools/attn_window_time.py [--mode bf16|pv8|qk8] [--anchors h,t] [--repeats 7] [--out profiles/attn_window_time.jsonl]
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

SHAPES = [dict(name="headline", B=3, H=16, hd=72, L_txt=512, N=1024, T=16, windows=(1, 2, 4, 16), inner=8),
          dict(name="long", B=1, H=16, hd=72, L_txt=512, N=3600, T=51, windows=(2, 8), inner=1)]
SHAPES_FP8 = [dict(name="11b", B=3, H=24, hd=128, L_txt=512, N=1024, T=16, windows=(1, 2, 4, 16), inner=8),
              dict(name="11b_long", B=1, H=24, hd=128, L_txt=512, N=3600, T=51, windows=(1, 2, 4, 51), inner=1)]


def time_arms(arms, warmup, repeats, inner):
    """every arm warmed up, then the arms alternate: `repeats` rounds of `inner` back-to-back calls between two device events"""
    for fn in arms.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    ms = {n_: [] for n_ in arms}
    for _ in range(repeats):
        for n_, fn in arms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(inner):
                fn()
            e1.record()
            e1.synchronize()
            ms[n_].append(e0.elapsed_time(e1) / inner)
    return ms


ANCHOR_WINDOWS = {"headline": (1, 2), "long": (2,)}


def time_anchors(a, s, _C, mmdit, dev, emit):
    """--anchors: full / window / anchored window as alternating arms, and the one-pass merge against two two-part passes"""
    head, tail = (int(x) for x in a.anchors.split(","))
    B, H, hd, Lt, N, T = s["B"], s["H"], s["hd"], s["L_txt"], s["N"], s["T"]
    L = Lt + N * T
    g = torch.Generator(device=dev).manual_seed(7)
    k = torch.randn(B, L, H * hd, device=dev, generator=g).to(torch.bfloat16)
    v = torch.randn(B, L, H * hd, device=dev, generator=g).to(torch.bfloat16)
    q = torch.randn(B, L, H * hd, device=dev, generator=g)
    kn = k.float().reshape(B, L, H, hd).norm(dim=-1).max()
    q = (q * (40.0 / float(q.reshape(B, L, H, hd).norm(dim=-1).max() * kn))).to(torch.bfloat16)   # prescaled, |q||k| <= ~40 < 56
    bound = float(q.float().reshape(B, L, H, hd).norm(dim=-1).max() * kn) * 1.01
    vt = torch.zeros(B, H, hd, (L + 63) // 64 * 64, dtype=torch.bfloat16, device=dev)
    _C.v_transpose(v, vt, H, hd)
    out = torch.empty_like(q)
    ws_full = _C.attention_workspace(dev)
    ws_win = _C.attention_window_workspace(B, H, L, hd, dev)
    ws_anc = _C.attention_window_anchor_workspace(B, H, L, hd, dev)
    n_prefix, n_suffix = mmdit.attention_window_bounds(Lt, N * T, N, head, tail)
    arms = {"full": lambda: _C.attention_fwd(q, k, vt, out, H, hd, hd ** -0.5, q_prescaled=True, workspace=ws_full, score_bound=bound)}
    fracs = {"full": 1.0}
    for w in ANCHOR_WINDOWS.get(s["name"], s["windows"][:1]):
        t = mmdit.attention_window_table(Lt, N * T, N, w)
        ta = mmdit.attention_window_table(Lt, N * T, N, w, anchor_head=head, anchor_tail=tail)
        arms[f"W{w}"] = (lambda t=t: _C.attention_fwd_window(q, k, vt, out, H, hd, hd ** -0.5, n_prefix=Lt, windows=t, q_prescaled=True,
                                                             score_bound=bound, workspace=ws_win))
        arms[f"W{w}a"] = (lambda ta=ta: _C.attention_fwd_window_anchor(q, k, vt, out, H, hd, hd ** -0.5, n_prefix=n_prefix, n_suffix=n_suffix,
                                                                       windows=ta, q_prescaled=True, score_bound=bound, workspace=ws_anc))
        fracs[f"W{w}"] = mmdit.window_tile_fraction(t, Lt, N * T)
        fracs[f"W{w}a"] = mmdit.window_tile_fraction(ta, Lt, N * T, (n_prefix, n_suffix))
    # the merge alone, on rows of this shape: one three-part pass against two two-part passes (values do not matter to the time)
    Lqp = (L + 255) // 256 * 256
    lse = torch.zeros(B, H, L, device=dev)
    ob, oc = torch.zeros(B, H, Lqp, hd, device=dev), torch.zeros(B, H, Lqp, hd, device=dev)
    lb, lc = torch.zeros(B, H, Lqp, device=dev), torch.zeros(B, H, Lqp, device=dev)
    arms["merge_2x_into"] = lambda: (_C.attention_merge_into(out, lse, ob, lb, H, hd), _C.attention_merge_into(out, lse, oc, lc, H, hd))
    arms["merge_into2"] = lambda: _C.attention_merge_into2(out, lse, ob, lb, oc, lc, H, hd)
    ms = time_arms(arms, a.warmup, a.repeats, s["inner"])
    med = {n_: statistics.median(x) for n_, x in ms.items()}
    for n_ in arms:
        row = dict(what="attn_window_anchor_time", shape=s["name"], B=B, H=H, hd=hd, L_txt=Lt, frame_tokens=N, frames=T, anchors=[head, tail],
                   n_prefix=n_prefix, n_suffix=n_suffix, arm=n_, repeats=a.repeats, calls_per_timing=s["inner"], ms=[round(x, 4) for x in ms[n_]],
                   median_ms=round(med[n_], 4), spread_ms=round(max(ms[n_]) - min(ms[n_]), 4), score_bound=round(bound, 3))
        if n_.startswith("merge"):
            row["time_ratio_to_two_passes"] = round(med[n_] / med["merge_2x_into"], 4)
        else:
            row["tile_fraction"] = round(fracs[n_], 4)
            row["time_ratio_to_full"] = round(med[n_] / med["full"], 4)
            if n_.endswith("a"):
                row["time_ratio_to_window"] = round(med[n_] / med[n_[:-1]], 4)
        emit(row)


def time_fp8(a, s, _C, mmdit, dev, emit):
    B, H, hd, Lt, N, T = s["B"], s["H"], s["hd"], s["L_txt"], s["N"], s["T"]
    L = Lt + N * T
    g = torch.Generator(device=dev).manual_seed(7)
    k = torch.randn(B, L, H * hd, device=dev, generator=g).to(torch.bfloat16)
    v = torch.randn(B, L, H * hd, device=dev, generator=g).to(torch.bfloat16)
    q = (torch.randn(B, L, H * hd, device=dev, generator=g) * (hd ** -0.5 * 1.4426950408889634)).to(torch.bfloat16)   # prescaled
    qk8 = a.mode == "qk8"
    vt8 = torch.zeros(B, H, _C.vt8_rows(hd), (L + 63) // 64 * 64, dtype=torch.uint8, device=dev)
    k8 = torch.zeros(_C.k8_shape(B, H, L, hd), dtype=torch.uint8, device=dev) if qk8 else None
    st = {}

    def pack():
        st["sv"] = _C.v_scale_fp8(v, H, hd)
        _C.v_transpose_fp8(v, st["sv"], vt8, H, hd)
        if qk8:
            st["sk"] = _C.v_scale_fp8(k, H, hd)
            _C.k_pack_fp8(k, st["sk"], k8, H, hd)

    pack()
    out = torch.empty_like(q)
    ws_full = _C.attention_workspace(dev)
    ws_win = _C.attention_window_workspace(B, H, L, hd, dev)
    tables = {w: mmdit.attention_window_table(Lt, N * T, N, w) for w in s["windows"]}

    def full():
        if qk8:
            _C.attention_fwd_qk8(q, k8, st["sk"], vt8, st["sv"], out, H, hd, hd ** -0.5, seg_len=L, q_prescaled=True, workspace=ws_full)
        else:
            _C.attention_fwd_pv8(q, k, vt8, st["sv"], out, H, hd, hd ** -0.5, q_prescaled=True, workspace=ws_full)

    def windowed(t):
        _C.attention_fwd_window_fp8(q, k8 if qk8 else k, st.get("sk"), vt8, st["sv"], out, H, hd, hd ** -0.5, n_prefix=Lt, windows=t,
                                    mode=a.mode, q_prescaled=True, workspace=ws_win, Lk=L)

    arms = {"full": full, "full+pack": lambda: (pack(), full())}
    for w, t in tables.items():
        arms[f"W{w}"] = lambda t=t: windowed(t)
        arms[f"W{w}+pack"] = lambda t=t: (pack(), windowed(t))
    ms = time_arms(arms, a.warmup, a.repeats, s["inner"])
    med = {n_: statistics.median(x) for n_, x in ms.items()}
    for n_ in arms:
        base = "full+pack" if n_.endswith("+pack") else "full"
        w = None if n_.startswith("full") else int(n_[1:].split("+")[0])
        frac = 1.0 if w is None else mmdit.window_tile_fraction(tables[w], Lt, N * T)
        ratio = med[n_] / med[base]
        emit(dict(what="attn_window_time", mode=a.mode, shape=s["name"], B=B, H=H, hd=hd, L_txt=Lt, frame_tokens=N, frames=T, arm=n_,
                  window_frames=w, with_packs=n_.endswith("+pack"), baseline_arm=base, repeats=a.repeats, calls_per_timing=s["inner"],
                  ms=[round(x, 4) for x in ms[n_]], median_ms=round(med[n_], 4), spread_ms=round(max(ms[n_]) - min(ms[n_]), 4),
                  tile_fraction=round(frac, 4), time_ratio=round(ratio, 4), time_ratio_over_tile_fraction=round(ratio / frac, 4)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--shapes", default=None, help="comma list; default: every shape of the mode")
    ap.add_argument("--mode", default="bf16", choices=("bf16", "pv8", "qk8"))
    ap.add_argument("--anchors", default=None, help="h,t: anchor frames (bf16 mode): anchored against un-anchored and full, merge A/B")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.repeats >= 3, "at least 3 rounds of every arm"

    from open_sora_amd import _C, mmdit

    dev = "cuda:0"
    torch.cuda.set_device(0)

    def emit(row):
        print(json.dumps(row), flush=True)
        if a.out:
            path = a.out if os.path.isabs(a.out) else os.path.join(ROOT, a.out)
            os.makedirs(os.path.dirname(path), exist_ok=True)
            with open(path, "a") as f:
                f.write(json.dumps(row) + "\n")

    for s in (SHAPES if a.mode == "bf16" else SHAPES_FP8):
        if a.shapes and s["name"] not in a.shapes.split(","):
            continue
        if a.mode != "bf16":
            assert a.anchors is None, "--anchors is timed in bf16 mode"
            time_fp8(a, s, _C, mmdit, dev, emit)
            continue
        if a.anchors:
            time_anchors(a, s, _C, mmdit, dev, emit)
            continue
        B, H, hd, Lt, N, T = s["B"], s["H"], s["hd"], s["L_txt"], s["N"], s["T"]
        L = Lt + N * T
        g = torch.Generator(device=dev).manual_seed(7)
        k = torch.randn(B, L, H * hd, device=dev, generator=g).to(torch.bfloat16)
        v = torch.randn(B, L, H * hd, device=dev, generator=g).to(torch.bfloat16)
        q = torch.randn(B, L, H * hd, device=dev, generator=g)
        kn = k.float().reshape(B, L, H, hd).norm(dim=-1).max()
        q = (q * (40.0 / float(q.reshape(B, L, H, hd).norm(dim=-1).max() * kn))).to(torch.bfloat16)   # prescaled, |q||k| <= ~40 < 56
        bound = float(q.float().reshape(B, L, H, hd).norm(dim=-1).max() * kn) * 1.01
        vt = torch.zeros(B, H, hd, (L + 63) // 64 * 64, dtype=torch.bfloat16, device=dev)
        _C.v_transpose(v, vt, H, hd)
        out = torch.empty_like(q)
        ws_full = _C.attention_workspace(dev)
        ws_win = _C.attention_window_workspace(B, H, L, hd, dev)
        tables = {w: mmdit.attention_window_table(Lt, N * T, N, w) for w in s["windows"]}
        arms = {"full": lambda: _C.attention_fwd(q, k, vt, out, H, hd, hd ** -0.5, q_prescaled=True, workspace=ws_full, score_bound=bound)}
        for w, t in tables.items():
            arms[f"W{w}"] = (lambda t=t: _C.attention_fwd_window(q, k, vt, out, H, hd, hd ** -0.5, n_prefix=Lt, windows=t, q_prescaled=True,
                                                                 score_bound=bound, workspace=ws_win))
        for fn in arms.values():
            for _ in range(a.warmup):
                fn()
        torch.cuda.synchronize()
        ms = {n_: [] for n_ in arms}
        for _ in range(a.repeats):
            for n_, fn in arms.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(s["inner"]):
                    fn()
                e1.record()
                e1.synchronize()
                ms[n_].append(e0.elapsed_time(e1) / s["inner"])
        med = {n_: statistics.median(x) for n_, x in ms.items()}
        rows_unit = _C.attention_launch_shape(B, H, L, 1, L, hd, bound, ws_full.numel()) if hasattr(_C, "attention_launch_shape") else None
        for n_ in arms:
            frac = 1.0 if n_ == "full" else mmdit.window_tile_fraction(tables[int(n_[1:])], Lt, N * T)
            ratio = med[n_] / med["full"]
            emit(dict(what="attn_window_time", shape=s["name"], B=B, H=H, hd=hd, L_txt=Lt, frame_tokens=N, frames=T, arm=n_,
                      window_frames=None if n_ == "full" else int(n_[1:]), repeats=a.repeats, calls_per_timing=s["inner"],
                      ms=[round(x, 4) for x in ms[n_]], median_ms=round(med[n_], 4), spread_ms=round(max(ms[n_]) - min(ms[n_]), 4),
                      tile_fraction=round(frac, 4), time_ratio=round(ratio, 4), time_ratio_over_tile_fraction=round(ratio / frac, 4),
                      full_call_launch_shape=str(rows_unit) if n_ == "full" else None, score_bound=round(bound, 3)))
        del q, k, v, vt, out


if __name__ == "__main__":
    main()
