"""Time the sampler's step cache (I2VDenoiser.denoise(step_cache=...), open_sora_amd/sampling.py) at the geometry of the bench.py
headline -- its model, latent frames and latent size, read from bench.py's own defaults; random weights as there -- on the shipped
schedule (50 steps, guidance 7.5 / 3.0, all three oscillation switches on), image-to-video, CFG triple.

Arms, alternating in ONE process after a warm-up loop of each; each timing is a host clock around a device synchronise:
  off      no keyword: the loop as it was before the step cache existed
  zero     step_cache=0.0: every step computed -- (a) the overhead of the head split, the distance and the residual store
  inf      step_cache=+inf: steps 1..N-2 skipped -- (b) a skipped step against a computed one, derived from the loop times
  half     every 2nd middle step skipped   } (c) forced patterns: with random weights the distances mean nothing, so the
  third    every 3rd middle step skipped   }     decision function is replaced by the pattern for these two arms
(d) each new kernel alone at the loop's shapes, with its byte count and achieved bandwidth; peak memory with the cache off / on.
The skip rate and the output quality on real checkpoints are NOT measured here or anywhere: no checkpoint is available.

    python tools/step_cache_time.py [--repeats 3] [--steps 50] [--out-dir profiles]

writes <out-dir>/step_cache_time.jsonl (one record per line) and <out-dir>/step_cache.md.

--sharded [--rank 3] [--sp-mode auto]: only the sequence-parallel arm (main_sharded): one rank of P = 8 at 512 text + 51 x 3,600 image
tokens (23,014 rows per rank), B = 1 and B = 3 -- a computed step against a skipped one, the step-cache kernels at the rank's
shapes, the sharded buffer sizes.  One GPU has no exchange: the transport is a stub that moves nothing (_StubTransport), so only the
rank's own kernels are timed.  Writes <out-dir>/step_cache_sp_time.jsonl and the section "Under sequence parallelism" of
<out-dir>/step_cache.md (the other sections are rendered from the step_cache_time.jsonl already there).
"""
from __future__ import annotations

import argparse
import json
import math
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

L_TXT = 512                    # bench.py, dit_line: the text length of the headline (a literal there)
SHIPPED = dict(guidance=7.5, guidance_img=3.0, text_osci=True, image_osci=True, scale_temporal_osci=True)
ARMS = ("off", "zero", "inf", "half", "third")


def headline_defaults():
    """bench.py's own argument defaults (model, latent frames, latent height = width)"""
    import bench

    argv, sys.argv = sys.argv, ["bench.py"]
    try:
        a = bench.parse()
    finally:
        sys.argv = argv
    return a.model, a.frames, a.latent_hw


def forced(period: int):
    """a stand-in for sampling.step_cache_decide: every `period`-th middle step skipped, the rest computed"""
    def decide(i, n_steps, d, acc, threshold, coefficients=None, have_rows=True):
        skip = 0 < i < n_steps - 1 and i % period == 0 and have_rows
        return (not skip), 0.0
    return decide


# --sharded: one rank of BASELINE configs[3] (XL, 512 text + 51 x 3,600 image tokens, P = 8: 23,014 rows per rank)
SP_P, SP_L_TXT, SP_N, SP_T = 8, 512, 3600, 51


class _StubTransport:
    """the transport of ONE rank with no peers: every collective returns at once and moves nothing, so the rank's kernels run on
    whatever its exchange buffers hold.  One GPU cannot run the exchange; this times the rank's own launches only."""

    def __init__(self, P: int, rank: int):
        self.P, self.rank, self.calls = P, rank, 0

    def _done(self, *a):
        from open_sora_amd import seqpar

        self.calls += 1
        return seqpar._Done()

    all_gather = all_to_all = all_reduce_max = _done


def main_sharded(a, out_dir):
    """one rank's computed step (step_head + step_distance + step_run) against its skipped step (step_head + step_distance +
    step_skip) at the rank shape of configs[3], B = 1 and B = 3, the arms alternating after a warm-up of each; then the step-cache
    kernels alone at the rank's shapes and the sharded buffer sizes"""
    from open_sora_amd import _C, configs, mmdit, sampling, seqpar

    jsonl = os.path.join(out_dir, "step_cache_sp_time.jsonl")
    open(jsonl, "w").close()
    rows = []

    def emit(row):
        rows.append(row)
        print(json.dumps(row), flush=True)
        with open(jsonl, "a") as f:
            f.write(json.dumps(row) + "\n")

    dev = "cuda:0"
    torch.cuda.set_device(0)
    cfg = dict(configs.MMDIT["XL"])
    torch.manual_seed(1234)
    model = mmdit.Flux(device_map=dev, torch_dtype=torch.bfloat16, **cfg)
    with torch.no_grad():
        for n_, p_ in model.named_parameters():
            if n_.startswith("cond_in"):
                p_.normal_(0, 0.02)
    hw = int(round((4 * SP_N) ** 0.5))
    assert (hw // 2) * (hw // 2) == SP_N
    L_img, D = SP_N * SP_T, cfg["hidden_size"]
    L = SP_L_TXT + L_img
    tp = _StubTransport(SP_P, a.rank)
    sp = seqpar.enable(model, mode=a.sp_mode, transport=tp)
    lo, hi = sp.shard_range(L, SP_L_TXT)
    rank_rows = hi - lo
    own_img = rank_rows - (min(hi, SP_L_TXT) - min(lo, SP_L_TXT))
    g = torch.Generator(device=dev).manual_seed(42)
    with torch.inference_mode():
        for B in (1, 3):
            z = torch.randn(1, 16, SP_T, hw, hw, device=dev, dtype=torch.bfloat16, generator=g)
            inp = dict(img=sampling.pack(z).repeat(B, 1, 1),
                       txt=(torch.randn(B, SP_L_TXT, cfg["context_in_dim"], device=dev, generator=g) * 0.2).to(torch.bfloat16),
                       y_vec=torch.randn(B, cfg["vec_in_dim"], device=dev, generator=g).to(torch.bfloat16),
                       timesteps=torch.full((B,), 0.7, device=dev, dtype=torch.bfloat16),
                       guidance=torch.full((B,), 7.5, device=dev, dtype=torch.bfloat16))
            inp["img_ids"], inp["txt_ids"] = sampling.prepare_ids(B, SP_T, hw, hw, SP_L_TXT, dev, torch.bfloat16)
            inp["cond"] = torch.randn(B, L_img, inp["img"].shape[2] + 4, device=dev, generator=g).to(torch.bfloat16)
            sc = model.step_cache_begin(1, B, L_img, dev, L_txt=SP_L_TXT)
            assert sc.prev.shape[1] == own_img

            def step(computed):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                st = model.step_head(sc, **inp)
                model.step_distance(sc)
                (model.step_run if computed else model.step_skip)(sc, st)
                torch.cuda.synchronize()
                return (time.perf_counter() - t0) * 1e3

            c0 = tp.calls
            step(True)                                  # warm-up of both arms (the computed step also stores the residual)
            calls_computed = tp.calls - c0
            c0 = tp.calls
            step(False)
            calls_skipped = tp.calls - c0
            ms = {"computed": [], "skipped": []}
            for _ in range(a.repeats):
                ms["computed"].append(round(step(True), 3))
                ms["skipped"].append(round(step(False), 3))
            med = {k: statistics.median(v) for k, v in ms.items()}
            emit(dict(what="step_cache_sp_step", model="XL", P=SP_P, rank=a.rank, sp_mode=a.sp_mode, head_exchange=sp.head_parallel(cfg["num_heads"]),
                      L_txt=SP_L_TXT, L_img=L_img, rank_rows=rank_rows, rank_image_rows=own_img, B=B, repeats=a.repeats, step_ms=ms,
                      median_ms={k: round(v, 3) for k, v in med.items()}, spread_ms={k: round(max(v) - min(v), 3) for k, v in ms.items()},
                      skipped_over_computed=round(med["skipped"] / med["computed"], 5),
                      stubbed_exchanges_per_step={"computed": calls_computed, "skipped": calls_skipped},
                      prev_bytes=sc.prev.numel() * 2, res_bytes=sc.res.numel() * 2,
                      single_device_prev_bytes=L_img * D * 2, single_device_res_bytes=B * L_img * D * 2))
            getattr(model, "_osk_ws_cache", {}).clear()
            sp._bufs.clear()
            object.__delattr__(model, "_osk_step_cache")
            del sc
            torch.cuda.empty_cache()
        # ---- the kernels alone at the rank's shapes
        joint = torch.randn(3, rank_rows, D, device=dev, generator=g).to(torch.bfloat16)
        t0_ = rank_rows - own_img
        xm, x3 = joint[:1, t0_:], joint[:, t0_:]
        prev = torch.randn(1, own_img, D, device=dev, generator=g).to(torch.bfloat16)
        res = torch.randn(3, own_img, D, device=dev, generator=g).to(torch.bfloat16)
        pairs, sums = torch.rand(SP_P, 2, device=dev), torch.zeros(2, device=dev)
        part = torch.empty(_C.step_delta_workspace_bytes(1, own_img, D), dtype=torch.uint8, device=dev)
        kernels = {"osk_step_delta_bf16": (lambda: _C.step_delta(xm, prev, pairs[a.rank], part), [1, own_img, D], 6 * own_img * D),
                   "osk_step_sums_combine_f32": (lambda: _C.step_sums_combine(pairs, sums), [SP_P, 2], 8 * SP_P + 8),
                   "osk_residual_sub_bf16": (lambda: _C.residual_sub(x3, res, res), [3, own_img, D], 6 * 3 * own_img * D),
                   "osk_residual_add_bf16": (lambda: _C.residual_add(x3, res, x3), [3, own_img, D], 6 * 3 * own_img * D),
                   "osk_copy_rows_bf16 (X saved)": (lambda: _C.copy_rows(x3, res), [3, own_img, D], 4 * 3 * own_img * D)}
        for name, (fn, shape, nbytes) in kernels.items():
            for _ in range(5):
                fn()
            times = []
            for _ in range(20):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                times.append(e0.elapsed_time(e1) * 1e3)
            us = statistics.median(times)
            emit(dict(what="step_cache_sp_kernel", kernel=name, shape=shape, bytes=nbytes, median_us=round(us, 2), min_us=round(min(times), 2),
                      max_us=round(max(times), 2), tb_per_s=round(nbytes / us * 1e-6, 3)))
    write_markdown(os.path.join(out_dir, "step_cache.md"), _read_jsonl(os.path.join(out_dir, "step_cache_time.jsonl")), rows)


def _read_jsonl(path: str) -> list:
    if not os.path.isfile(path):
        return []
    with open(path) as f:
        return [json.loads(ln) for ln in f if ln.strip()]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup-steps", type=int, default=6)
    ap.add_argument("--out-dir", default="profiles")
    ap.add_argument("--sharded", action="store_true", help="only the sharded arm: one sequence-parallel rank's step, transport stubbed")
    ap.add_argument("--rank", type=int, default=3, help="the sharded arm's rank (a middle rank: no text rows)")
    ap.add_argument("--sp-mode", default="auto", help="the sharded arm's exchange mode (seqpar.enable(mode=...))")
    a = ap.parse_args()
    assert a.repeats >= 3, "at least 3 repeats of each arm"
    out_dir = a.out_dir if os.path.isabs(a.out_dir) else os.path.join(ROOT, a.out_dir)
    os.makedirs(out_dir, exist_ok=True)
    if a.sharded:
        return main_sharded(a, out_dir)
    jsonl = os.path.join(out_dir, "step_cache_time.jsonl")
    open(jsonl, "w").close()

    from open_sora_amd import _C, configs, mmdit, sampling

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
    masks = torch.zeros(1, 1, T, hw, hw, device=dev, dtype=torch.bfloat16)
    masks[:, :, 0] = 1                                       # the first latent frame is given
    ref = torch.randn(1, 16, T, hw, hw, device=dev, generator=g).to(torch.bfloat16) * masks
    x0 = sampling.pack(z).repeat(3, 1, 1)
    L_img, D = x0.shape[1], cfg["hidden_size"]
    den = sampling.I2VDenoiser()
    real_decide = sampling.step_cache_decide

    def loop(arm, steps):
        ts = sampling.get_schedule(steps, (hw // 2) * (hw // 2), T)
        extra = {} if arm == "off" else {"step_cache": math.inf if arm == "inf" else 0.0}
        sampling.step_cache_decide = forced(2) if arm == "half" else forced(3) if arm == "third" else real_decide
        try:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            den.denoise(model, img=x0, timesteps=ts, img_ids=img_ids, txt_ids=txt_ids, masks=masks, masked_ref=ref, txt=txt, y_vec=y_vec,
                        **extra, **SHIPPED)
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t0) * 1e3
        finally:
            sampling.step_cache_decide = real_decide
        rec = den.last_step_cache
        return ms, (None if rec is None else sum(1 for _, _, c in rec if not c))

    rows = []

    def emit(row):
        rows.append(row)
        print(json.dumps(row), flush=True)
        with open(jsonl, "a") as f:
            f.write(json.dumps(row) + "\n")

    with torch.inference_mode():
        # ---- peak memory, cache off and on, each from an empty workspace cache (also the first touch of every kernel and plan)
        peak = {}
        for arm in ("off", "inf"):
            getattr(model, "_osk_ws_cache", {}).clear()
            if hasattr(model, "_osk_step_cache"):
                object.__delattr__(model, "_osk_step_cache")
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            torch.cuda.reset_peak_memory_stats()
            loop(arm, a.warmup_steps)
            peak[arm] = torch.cuda.max_memory_allocated()
        for arm in ARMS:
            loop(arm, a.warmup_steps)
        ms = {arm: [] for arm in ARMS}
        skipped = {}
        for _ in range(a.repeats):
            for arm in ARMS:
                t, skipped[arm] = loop(arm, a.steps)
                ms[arm].append(round(t, 2))
        med = {k: statistics.median(v) for k, v in ms.items()}
        N = a.steps
        computed_ms = med["zero"] / N
        skipped_ms = (med["inf"] - 2 * computed_ms) / max(N - 2, 1)
        emit(dict(what="step_cache_loop", model=model_name, frames=T, latent_hw=hw, L_img=L_img, L_txt=L_TXT, steps=N, repeats=a.repeats,
                  loop_ms={k: v for k, v in ms.items()}, median_ms={k: round(v, 2) for k, v in med.items()},
                  spread_ms={k: round(max(v) - min(v), 2) for k, v in ms.items()}, skipped_steps=skipped,
                  a_zero_over_off=round(med["zero"] / med["off"], 4), overhead_ms_per_step=round((med["zero"] - med["off"]) / N, 3),
                  b_computed_step_ms=round(computed_ms, 2), b_skipped_step_ms=round(skipped_ms, 2),
                  b_skipped_over_computed=round(skipped_ms / computed_ms, 4),
                  c_half_over_off=round(med["half"] / med["off"], 4), c_third_over_off=round(med["third"] / med["off"], 4),
                  peak_mem_off_bytes=peak["off"], peak_mem_on_bytes=peak["inf"], extra_peak_mem_bytes=peak["inf"] - peak["off"]))

        # ---- (d) the new kernels alone, at the loop's shapes: M of the conditional row as block 0 leaves it (a view of the joint
        # buffer), the residual of the triple
        joint = torch.randn(3, L_TXT + L_img, D, device=dev, generator=g).to(torch.bfloat16)
        xm = joint[:1, L_TXT:]
        prev = torch.randn(1, L_img, D, device=dev, generator=g).to(torch.bfloat16)
        res = torch.randn(3, L_img, D, device=dev, generator=g).to(torch.bfloat16)
        sums = torch.zeros(2, device=dev)
        part = torch.empty(_C.step_delta_workspace_bytes(1, L_img, D), dtype=torch.uint8, device=dev)
        x3 = joint[:, L_TXT:]
        kernels = {"osk_step_delta_bf16": (lambda: _C.step_delta(xm, prev, sums, part), 6 * L_img * D),
                   "osk_residual_sub_bf16": (lambda: _C.residual_sub(x3, res, res), 6 * 3 * L_img * D),
                   "osk_residual_add_bf16": (lambda: _C.residual_add(x3, res, x3), 6 * 3 * L_img * D),
                   "osk_copy_rows_bf16 (X saved)": (lambda: _C.copy_rows(x3, res), 4 * 3 * L_img * D)}
        for name, (fn, nbytes) in kernels.items():
            for _ in range(5):
                fn()
            times = []
            for _ in range(20):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                times.append(e0.elapsed_time(e1) * 1e3)
            us = statistics.median(times)
            emit(dict(what="step_cache_kernel", kernel=name, shape=[1 if "delta" in name else 3, L_img, D], bytes=nbytes,
                      median_us=round(us, 2), min_us=round(min(times), 2), max_us=round(max(times), 2), tb_per_s=round(nbytes / us * 1e-6, 3)))
    write_markdown(os.path.join(out_dir, "step_cache.md"), rows, _read_jsonl(os.path.join(out_dir, "step_cache_sp_time.jsonl")))


def write_markdown(path: str, rows: list, sp_rows: list = ()) -> None:
    lp = next(r for r in rows if r["what"] == "step_cache_loop")
    ks = [r for r in rows if r["what"] == "step_cache_kernel"]
    m, sp = lp["median_ms"], lp["spread_ms"]
    lines = [
        "# Step cache: the sampling loop with the block stack skipped on some steps",
        "",
        "`I2VDenoiser.denoise(step_cache=threshold)` (DESIGN.md section 4).  Written by `tools/step_cache_time.py`; the records are in",
        "`profiles/step_cache_time.jsonl`.  One MI355X, one process, the arms alternating; host clock around a device synchronise.",
        f"Model {lp['model']}, {lp['L_img']} image + {lp['L_txt']} text tokens, CFG triple, {lp['steps']} steps of the shipped schedule, random weights,",
        f"{lp['repeats']} repeats of each arm (median; spread = max - min).",
        "",
        "| arm | loop ms (median) | spread ms | skipped steps | over `off` |",
        "|---|---|---|---|---|",
    ]
    for arm, note in (("off", "no keyword"), ("zero", "`step_cache=0.0`, every step computed"), ("inf", "`step_cache=inf`, steps 1..N-2 skipped"),
                      ("half", "forced: every 2nd middle step skipped"), ("third", "forced: every 3rd middle step skipped")):
        lines.append(f"| {arm} ({note}) | {m[arm]} | {sp[arm]} | {lp['skipped_steps'][arm]} | {round(m[arm] / m['off'], 4)} |")
    lines += [
        "",
        f"(a) overhead of the head split, the distance and the residual store: zero / off = {lp['a_zero_over_off']}, "
        f"{lp['overhead_ms_per_step']} ms per step (one host synchronisation per step included).",
        f"(b) one computed step {lp['b_computed_step_ms']} ms (zero / N); one skipped step {lp['b_skipped_step_ms']} ms ((inf - 2 computed) / (N - 2)): "
        f"skipped / computed = {lp['b_skipped_over_computed']}.",
        f"(c) forced patterns: every 2nd middle step skipped {lp['c_half_over_off']} of the off loop, every 3rd {lp['c_third_over_off']}.",
        f"Peak memory (torch.cuda.max_memory_allocated): off {lp['peak_mem_off_bytes'] / 2 ** 20:.0f} MiB, on {lp['peak_mem_on_bytes'] / 2 ** 20:.0f} MiB "
        f"(+{lp['extra_peak_mem_bytes'] / 2 ** 20:.0f} MiB: M of the conditional rows and R of every row).",
        "",
        "(d) the new kernels alone at the loop's shapes (20 launches each, device events):",
        "",
        "| kernel | shape | bytes | median us | TB/s |",
        "|---|---|---|---|---|",
    ]
    for r in ks:
        lines.append(f"| {r['kernel']} | {r['shape']} | {r['bytes']} | {r['median_us']} | {r['tb_per_s']} |")
    lines += [
        "",
        "NOT measured: the skip rate a threshold gives and the output quality of skipped steps on real checkpoints -- the weights here",
        "are random, so the natural distances carry no meaning (hence the forced patterns), and no calibrated polynomial ships.",
        "",
    ]
    lines += sharded_markdown(list(sp_rows))
    with open(path, "w") as f:
        f.write("\n".join(lines))


def sharded_markdown(sp_rows: list) -> list:
    """the section of the --sharded arm (records of profiles/step_cache_sp_time.jsonl); empty without records"""
    steps = [r for r in sp_rows if r["what"] == "step_cache_sp_step"]
    ks = [r for r in sp_rows if r["what"] == "step_cache_sp_kernel"]
    if not steps:
        return []
    s0 = steps[0]
    lines = [
        "## Under sequence parallelism: one rank's step",
        "",
        "`tools/step_cache_time.py --sharded`; the records are in `profiles/step_cache_sp_time.jsonl`.  One rank of BASELINE configs[3]:",
        f"model {s0['model']}, {s0['L_txt']} text + {s0['L_img']} image tokens over P = {s0['P']}, rank {s0['rank']} with {s0['rank_rows']} rows "
        f"({s0['rank_image_rows']} of them image rows), exchange mode `{s0['sp_mode']}` ({'head exchange' if s0['head_exchange'] else 'all-gather'}),",
        "random weights, ONE MI355X.  The exchange does not exist on one GPU: the transport is a stub whose collectives return at once and move",
        "nothing, so the times are the rank's own kernels on whatever its exchange buffers hold -- K / V exchange, the 8-byte gather of",
        "the sums and the gather of the prediction cost nothing here.  A step = `step_head` + `step_distance` (the 8-byte read back) +",
        f"`step_run` or `step_skip`; host clock around a device synchronise, the two arms alternating, {s0['repeats']} repeats (median; spread = max - min).",
        "",
        "| B | computed step ms | spread | skipped step ms | spread | skipped / computed | stubbed exchanges computed / skipped |",
        "|---|---|---|---|---|---|---|",
    ]
    for r in steps:
        m, sp, ex = r["median_ms"], r["spread_ms"], r["stubbed_exchanges_per_step"]
        lines.append(f"| {r['B']} | {m['computed']} | {sp['computed']} | {m['skipped']} | {sp['skipped']} | {r['skipped_over_computed']} | "
                     f"{ex['computed']} / {ex['skipped']} |")
    lines += ["", "Sharded buffers of the cache on this rank (bf16; the single-device cache of the same sequence in brackets):", ""]
    for r in steps:
        lines.append(f"- B = {r['B']}: `prev` {r['prev_bytes'] / 2 ** 20:.1f} MiB ({r['single_device_prev_bytes'] / 2 ** 20:.1f} MiB), "
                     f"`res` {r['res_bytes'] / 2 ** 20:.1f} MiB ({r['single_device_res_bytes'] / 2 ** 20:.1f} MiB), `pairs` {8 * r['P']} bytes.")
    lines += ["", "The step-cache kernels alone at the rank's shapes (20 launches each, device events; the combine is one lane, latency only):", "",
              "| kernel | shape | bytes | median us | TB/s |", "|---|---|---|---|---|"]
    for r in ks:
        lines.append(f"| {r['kernel']} | {r['shape']} | {r['bytes']} | {r['median_us']} | {r['tb_per_s']} |")
    lines += [
        "",
        "NOT measured: the exchange of the sums (and every other exchange) on a real multi-GPU node, the skip rate a threshold gives and",
        "the output quality.  No threshold is set on these numbers.",
        "",
    ]
    return lines


if __name__ == "__main__":
    main()
