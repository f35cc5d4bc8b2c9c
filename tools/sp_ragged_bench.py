"""One sequence-parallel rank's exchange-free attention on a ragged split against the nearest divisible length
(profiles/sp_ragged.md): 256 px, 16:9, 129 frames -- L = 8,828 over P = 8 ranks (7 x 1,104 + 1,100 keys, 1,104 query rows) through
osk_attention_fwd_ragged_bf16, and L = 8,832 (8 x 1,104) through the single launch.  Both head dims (XL: 72 x 16 heads, 11B: 128 x 24),
B = 1, bounded body.  The two calls alternate in one process; per call: 5 warm-ups, then the median of 40 event-timed launches."""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from open_sora_amd import _C  # noqa: E402

LOG2E = 1.4426950408889634


def unit_rms(t, H, hd):
    t = t.view(*t.shape[:-1], H, hd)
    return (t * torch.rsqrt(t.pow(2).mean(-1, keepdim=True) + 1e-6)).reshape(*t.shape[:-2], H * hd)


def timed(fn, n=40, warm=5):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return statistics.median(ts), min(ts), max(ts)


def main():
    P, Lc, Ltail = 8, 1104, 1100
    out = []
    for hd, H in ((72, 16), (128, 24)):
        D, Lp = H * hd, (Lc + 63) // 64 * 64
        g = torch.Generator(device="cuda").manual_seed(1)
        q = (unit_rms(torch.randn(1, Lc, D, device="cuda", generator=g), H, hd) * (hd ** -0.5 * LOG2E)).to(torch.bfloat16)
        k = unit_rms(torch.randn(P, 1, Lc, D, device="cuda", generator=g), H, hd).to(torch.bfloat16)
        v = torch.randn(P, 1, Lc, D, device="cuda", generator=g).to(torch.bfloat16)
        bound = 1.02 * q.float().view(1, Lc, H, hd).norm(dim=-1).amax().item() * k.float().view(P, 1, Lc, H, hd).norm(dim=-1).amax().item()
        vt = torch.zeros(P, 1, H, hd, Lp, dtype=torch.bfloat16, device="cuda")
        _C.v_transpose(v.view(P, Lc, D), vt.view(P, H, hd, Lp), H, hd)
        vt_r = vt.clone()
        vt_r[-1].zero_()
        _C.v_transpose(v[-1][:, :Ltail], vt_r[-1].reshape(-1)[: H * hd * ((Ltail + 63) // 64 * 64)].view(1, H, hd, -1), H, hd)
        o = torch.empty(1, Lc, D, dtype=torch.bfloat16, device="cuda")
        ws, wsr = _C.attention_workspace("cuda"), _C.attention_ragged_workspace(1, H, Lc, hd, "cuda")
        kw = dict(k_seg_stride=k.stride(0), q_prescaled=True, score_bound=bound)
        single = lambda: _C.attention_fwd(q, k[0], vt, o, H, hd, hd ** -0.5, n_seg=P, seg_len=Lc, vt_seg_stride=vt.stride(0), workspace=ws, **kw)
        ragged = lambda: _C.attention_fwd_ragged(q, k[0], vt_r, o, H, hd, hd ** -0.5, n_seg=P, seg_len=Lc, last_seg_len=Ltail,
                                                 vt_seg_stride=vt_r.stride(0), workspace=wsr, **kw)
        full7 = lambda: _C.attention_fwd(q, k[0], vt, o, H, hd, hd ** -0.5, n_seg=P - 1, seg_len=Lc, vt_seg_stride=vt.stride(0), workspace=ws, **kw)
        rec = dict(hd=hd, H=H, Lq=Lc, body_single=_C.attention_body(hd, P, Lc, bound), launch_shape_single=_C.attention_launch_shape(1, H, Lc, P, Lc, hd, bound, ws.numel()),
                   launch_shape_7seg=_C.attention_launch_shape(1, H, Lc, P - 1, Lc, hd, bound, ws.numel()))
        for rnd in range(2):          # alternate: a drift of the clocks shows as a difference between the rounds
            for name, fn in (("single_8832", single), ("ragged_8828", ragged), ("launch_a_alone_7x1104", full7)):
                med, lo, hi = timed(fn)
                rec[f"{name}_ms_round{rnd}"] = dict(median=round(med, 4), min=round(lo, 4), max=round(hi, 4))
        rec["ratio_ragged_over_single"] = round(min(rec[f"ragged_8828_ms_round{r}"]["median"] for r in range(2)) /
                                                min(rec[f"single_8832_ms_round{r}"]["median"] for r in range(2)), 4)
        print(json.dumps(rec))
        out.append(rec)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
