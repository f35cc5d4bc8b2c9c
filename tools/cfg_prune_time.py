"""Time the whole sampling loop with and without CFG branch pruning (I2VDenoiser.denoise(cfg_prune=...), open_sora_amd/sampling.py)
at the geometry of the bench.py headline -- its model, latent frames and latent size, read from bench.py's own defaults; random
weights as there -- on the shipped schedule: 50 steps, guidance 7.5 / 3.0, all three oscillation switches on
(configs/diffusion/inference/256px.py:20-28 of the reference).  Two workloads:

  i2v   a non-zero first-frame condition: the triple everywhere but the 20 steps whose guidances are both 1.0 (one branch);
  t2v   no condition, the two negative prompts equal: two branches, one on those 20 steps.

Expectations from the README's per-step numbers (127.1 ms at CFG batch 3, 47.4 ms at batch 1): i2v (30 x 127.1 + 20 x 47.4) /
(50 x 127.1) = 0.75 of the unpruned loop; t2v 80 branch forwards in place of 150.

Both arms run in ONE process, alternating, after a warm-up loop of each (14 steps: every branch count of the arm); each timing is a
host clock around a device synchronise.  Peak memory (torch.cuda.max_memory_allocated) is taken per arm in a phase of its own, from
an empty workspace cache: the pruned arm keeps one activation workspace set per batch size in use, the unpruned arm one.

    python tools/cfg_prune_time.py [--repeats 3] [--steps 50] [--out profiles/cfg_prune_time.jsonl]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

L_TXT = 512                    # bench.py, dit_line: the text length of the headline (a literal there)
SHIPPED = dict(guidance=7.5, guidance_img=3.0, text_osci=True, image_osci=True, scale_temporal_osci=True)
STEP_MS_B3, STEP_MS_B1 = 127.1, 47.4     # README: the XL step at CFG batch 3 and at batch 1


def headline_defaults():
    """bench.py's own argument defaults (model, latent frames, latent height = width)"""
    import bench

    argv, sys.argv = sys.argv, ["bench.py"]
    try:
        a = bench.parse()
    finally:
        sys.argv = argv
    return a.model, a.frames, a.latent_hw


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup-steps", type=int, default=14)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.repeats >= 3, "at least 3 repeats of each arm"

    from open_sora_amd import configs, mmdit, sampling

    model_name, T, hw = headline_defaults()
    dev = "cuda:0"
    torch.cuda.set_device(0)
    cfg = dict(configs.MMDIT[model_name])
    torch.manual_seed(1234)
    model = mmdit.Flux(device_map=dev, torch_dtype=torch.bfloat16, **cfg)
    with torch.no_grad():  # random-init weights of the architecture, as bench.py (cond_in is zero-init in the reference)
        for n_, p_ in model.named_parameters():
            if n_.startswith("cond_in"):
                p_.normal_(0, 0.02)
    g = torch.Generator(device=dev).manual_seed(42)
    z = torch.randn(1, 16, T, hw, hw, device=dev, dtype=torch.bfloat16, generator=g)
    txt = (torch.randn(3, L_TXT, cfg["context_in_dim"], device=dev, generator=g) * 0.2).to(torch.bfloat16)
    y_vec = torch.randn(3, cfg["vec_in_dim"], device=dev, generator=g).to(torch.bfloat16)
    img_ids, txt_ids = sampling.prepare_ids(3, T, hw, hw, L_TXT, dev, torch.bfloat16)
    zeros = lambda ch: torch.zeros(1, ch, T, hw, hw, device=dev, dtype=torch.bfloat16)
    masks_i2v = zeros(1)
    masks_i2v[:, :, 0] = 1                                   # the first latent frame is given
    ref_i2v = torch.randn(1, 16, T, hw, hw, device=dev, generator=g).to(torch.bfloat16) * masks_i2v
    txt_t2v, y_t2v = txt.clone(), y_vec.clone()              # prepare_guidance: text + neg + neg
    txt_t2v[2:], y_t2v[2:] = txt_t2v[1:2], y_t2v[1:2]
    workloads = {"i2v": dict(masks=masks_i2v, masked_ref=ref_i2v, txt=txt, y_vec=y_vec),
                 "t2v": dict(masks=zeros(1), masked_ref=zeros(16), txt=txt_t2v, y_vec=y_t2v)}
    x0 = sampling.pack(z).repeat(3, 1, 1)
    den = sampling.I2VDenoiser()

    def loop(w, prune, steps):
        ts = sampling.get_schedule(steps, (hw // 2) * (hw // 2), T)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        den.denoise(model, img=x0, timesteps=ts, img_ids=img_ids, txt_ids=txt_ids, cfg_prune=prune, **workloads[w], **SHIPPED)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, list(den.last_branch_counts)

    def emit(row):
        print(json.dumps(row), flush=True)
        if a.out:
            path = a.out if os.path.isabs(a.out) else os.path.join(ROOT, a.out)
            os.makedirs(os.path.dirname(path), exist_ok=True)
            with open(path, "a") as f:
                f.write(json.dumps(row) + "\n")

    with torch.inference_mode():
        for w in workloads:
            # ---- peak memory per arm, each from an empty workspace cache (also the first touch of every kernel and plan)
            peak = {}
            for prune in (False, True):
                getattr(model, "_osk_ws_cache", {}).clear()
                torch.cuda.synchronize()
                torch.cuda.empty_cache()
                torch.cuda.reset_peak_memory_stats()
                base = torch.cuda.memory_allocated()
                loop(w, prune, a.warmup_steps)
                peak[prune] = (torch.cuda.max_memory_allocated(), base)
            # ---- warm-up of both arms with every workspace set in place, then the alternating timed repeats
            for prune in (False, True):
                loop(w, prune, a.warmup_steps)
            ms = {False: [], True: []}
            counts = {}
            for _ in range(a.repeats):
                for prune in (False, True):
                    t, counts[prune] = loop(w, prune, a.steps)
                    ms[prune].append(round(t, 2))
            med = {k: statistics.median(v) for k, v in ms.items()}
            spread = {k: round(max(v) - min(v), 2) for k, v in ms.items()}
            c = counts[True]
            n1, n2, n3 = c.count(1), c.count(2), c.count(3)
            row = dict(what="cfg_prune_loop", workload=w, model=model_name, frames=T, latent_hw=hw, L_txt=L_TXT, steps=a.steps,
                       repeats=a.repeats, branch_counts={"1": n1, "2": n2, "3": n3}, branch_forwards_pruned=sum(c),
                       branch_forwards_unpruned=3 * len(c), unpruned_ms=ms[False], pruned_ms=ms[True],
                       unpruned_median_ms=round(med[False], 2), pruned_median_ms=round(med[True], 2),
                       unpruned_spread_ms=spread[False], pruned_spread_ms=spread[True],
                       ratio=round(med[True] / med[False], 4), forwards_ratio=round(sum(c) / (3 * len(c)), 4),
                       faster_by_ms=round(med[False] - med[True], 2),
                       faster_by_more_than_unpruned_spread=bool(max(ms[True]) < min(ms[False]) and med[False] - med[True] > spread[False]),
                       peak_mem_unpruned_bytes=peak[False][0], peak_mem_pruned_bytes=peak[True][0], mem_before_loop_bytes=peak[False][1],
                       extra_peak_mem_pruned_bytes=peak[True][0] - peak[False][0])
            if w == "i2v" and a.steps == 50:
                row["ratio_expected_from_readme"] = round((n3 * STEP_MS_B3 + n1 * STEP_MS_B1) / (len(c) * STEP_MS_B3), 4)
            emit(row)


if __name__ == "__main__":
    main()
