"""Time the sampler's attention broadcast (I2VDenoiser.denoise(attn_broadcast=...), open_sora_amd/sampling.py) at the geometry of the
bench.py headline -- its model, latent frames and latent size, read from bench.py's own defaults; random weights as there -- on the
shipped schedule (50 steps, guidance 7.5 / 3.0, all three oscillation switches on), image-to-video, CFG triple.

One process, the arms alternating after a warm-up of each; each timing is a host clock around a device synchronise:
  (a) loops   off (no keyword) | off_kw (attn_broadcast=None) | i2 | i3 (interval 2 / 3, default range)        -- (a) and (d)
  (b, c) one forward_ckpt at B = 3: plain | store | reuse                                                         -- the price of the
      copies, and what a reuse step costs; next to it the arithmetic from the kernel profile
  (e) peak memory of a loop with and without, each from an empty workspace cache; the cache size as arithmetic
  the copy kernel alone at the loop's shapes, store and load, with its byte count and achieved bandwidth
--sharded: one rank of P = 8 at 512 text + 51 x 3,600 image tokens, the transport stubbed as tools/step_cache_time.py --sharded does:
  plain | store | reuse forward of the rank, B = 1 and B = 3, and the stubbed exchanges each makes.
Output quality on real checkpoints and the exchange saved on a multi-GPU node are NOT measured here or anywhere.

    python tools/attn_broadcast_time.py [--repeats 3] [--steps 50] [--sharded] [--out-dir profiles]

writes <out-dir>/attn_broadcast.jsonl (appends the sharded records with --sharded) and <out-dir>/attn_broadcast.md.
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

from tools.step_cache_time import L_TXT, SHIPPED, SP_L_TXT, SP_N, SP_P, SP_T, _StubTransport, _read_jsonl, headline_defaults   # noqa: E402

# the kernel profile of the headline step the issue quotes (profiles/r06g_step_kernel_stats.csv), ms of a 128 ms step
PROFILE = dict(step=128.0, attention=84.5, linears=40.0, qkv_share_of_linears=0.25, qknorm_rope=2.3)
LOOP_ARMS = ("off", "off_kw", "i2", "i3")
STEP_ARMS = ("plain", "store", "reuse")


def _model(name):
    from open_sora_amd import configs, mmdit

    cfg = dict(configs.MMDIT[name])
    torch.manual_seed(1234)
    model = mmdit.Flux(device_map="cuda:0", torch_dtype=torch.bfloat16, **cfg)
    with torch.no_grad():  # random-init weights of the architecture, as bench.py (cond_in is zero-init in the reference)
        for n_, p_ in model.named_parameters():
            if n_.startswith("cond_in"):
                p_.normal_(0, 0.02)
    return cfg, model


def _inputs(cfg, B, T, hw, L_txt, g):
    from open_sora_amd import sampling

    dev = "cuda:0"
    z = torch.randn(1, 16, T, hw, hw, device=dev, dtype=torch.bfloat16, generator=g)
    inp = dict(img=sampling.pack(z).repeat(B, 1, 1),
               txt=(torch.randn(B, L_txt, cfg["context_in_dim"], device=dev, generator=g) * 0.2).to(torch.bfloat16),
               y_vec=torch.randn(B, cfg["vec_in_dim"], device=dev, generator=g).to(torch.bfloat16),
               timesteps=torch.full((B,), 0.7, device=dev, dtype=torch.bfloat16), guidance=torch.full((B,), 7.5, device=dev, dtype=torch.bfloat16))
    inp["img_ids"], inp["txt_ids"] = sampling.prepare_ids(B, T, hw, hw, L_txt, dev, torch.bfloat16)
    inp["cond"] = torch.randn(B, inp["img"].shape[1], inp["img"].shape[2] + 4, device=dev, generator=g).to(torch.bfloat16)
    return inp


def _time_steps(model, inp, ac, rows, repeats):
    """plain | store | reuse forward, alternating after a warm-up of each -> {arm: [ms]}"""
    def step(arm):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        model(**inp, **({} if arm == "plain" else {"attn_cache": (ac, arm, rows)}))
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    for arm in STEP_ARMS:
        step(arm)
    ms = {arm: [] for arm in STEP_ARMS}
    for _ in range(repeats):
        for arm in STEP_ARMS:
            ms[arm].append(round(step(arm), 3))
    return ms


def _emitter(jsonl, rows):
    def emit(row):
        rows.append(row)
        print(json.dumps(row), flush=True)
        with open(jsonl, "a") as f:
            f.write(json.dumps(row) + "\n")
    return emit


def cache_bytes(cfg, rows, L):
    return (cfg["depth"] + cfg["depth_single_blocks"]) * rows * L * cfg["hidden_size"] * 2


def main_sharded(a, out_dir, jsonl):
    from open_sora_amd import seqpar

    rows = []
    emit = _emitter(jsonl, rows)
    torch.cuda.set_device(0)
    cfg, model = _model("XL")
    hw = int(round((4 * SP_N) ** 0.5))
    L = SP_L_TXT + SP_N * SP_T
    tp = _StubTransport(SP_P, a.rank)
    sp = seqpar.enable(model, mode=a.sp_mode, transport=tp)
    g = torch.Generator(device="cuda:0").manual_seed(42)
    with torch.inference_mode():
        for B in (1, 3):
            inp = _inputs(cfg, B, SP_T, hw, SP_L_TXT, g)
            ac = model.attention_broadcast_begin(B, SP_L_TXT, SP_N * SP_T, "cuda:0")
            calls = {}
            for arm in STEP_ARMS:                      # (also the warm-up; store before reuse)
                c0 = tp.calls
                model(**inp, **({} if arm == "plain" else {"attn_cache": (ac, arm, tuple(range(B)))}))
                calls[arm] = tp.calls - c0
            ms = _time_steps(model, inp, ac, tuple(range(B)), a.repeats)
            med = {k: statistics.median(v) for k, v in ms.items()}
            emit(dict(what="attn_broadcast_sp_step", model="XL", P=SP_P, rank=a.rank, sp_mode=a.sp_mode, head_exchange=sp.head_parallel(cfg["num_heads"]),
                      L_txt=SP_L_TXT, L_img=SP_N * SP_T, rank_rows=ac.L, B=B, repeats=a.repeats, step_ms=ms,
                      median_ms={k: round(v, 3) for k, v in med.items()}, spread_ms={k: round(max(v) - min(v), 3) for k, v in ms.items()},
                      store_over_plain=round(med["store"] / med["plain"], 5), reuse_over_plain=round(med["reuse"] / med["plain"], 5),
                      stubbed_exchanges_per_step=calls, cache_bytes=ac.slots.numel() * 2, single_device_cache_bytes=cache_bytes(cfg, B, L)))
            getattr(model, "_osk_ws_cache", {}).clear()
            sp._bufs.clear()
            object.__delattr__(model, "_osk_attn_cache")
            del ac
            torch.cuda.empty_cache()
    write_markdown(os.path.join(out_dir, "attn_broadcast.md"), _read_jsonl(jsonl))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup-steps", type=int, default=6)
    ap.add_argument("--out-dir", default="profiles")
    ap.add_argument("--sharded", action="store_true", help="only the sharded arm: one sequence-parallel rank's forward, transport stubbed")
    ap.add_argument("--rank", type=int, default=3, help="the sharded arm's rank (a middle rank: no text rows)")
    ap.add_argument("--sp-mode", default="auto", help="the sharded arm's exchange mode (seqpar.enable(mode=...))")
    a = ap.parse_args()
    assert a.repeats >= 3, "at least 3 repeats of each arm"
    out_dir = a.out_dir if os.path.isabs(a.out_dir) else os.path.join(ROOT, a.out_dir)
    os.makedirs(out_dir, exist_ok=True)
    jsonl = os.path.join(out_dir, "attn_broadcast.jsonl")
    if a.sharded:
        keep = [r for r in _read_jsonl(jsonl) if not r["what"].startswith("attn_broadcast_sp")]
        with open(jsonl, "w") as f:
            f.writelines(json.dumps(r) + "\n" for r in keep)
        return main_sharded(a, out_dir, jsonl)
    open(jsonl, "w").close()

    from open_sora_amd import _C, configs, sampling

    model_name, T, hw = headline_defaults()
    dev = "cuda:0"
    torch.cuda.set_device(0)
    cfg, model = _model(model_name)
    g = torch.Generator(device=dev).manual_seed(42)
    inp = _inputs(cfg, 3, T, hw, L_TXT, g)
    masks = torch.zeros(1, 1, T, hw, hw, device=dev, dtype=torch.bfloat16)
    masks[:, :, 0] = 1                                       # the first latent frame is given
    ref = torch.randn(1, 16, T, hw, hw, device=dev, generator=g).to(torch.bfloat16) * masks
    L_img, D = inp["img"].shape[1], cfg["hidden_size"]
    L = L_TXT + L_img
    den = sampling.I2VDenoiser()
    rows = []
    emit = _emitter(jsonl, rows)

    def loop(arm, steps):
        ts = sampling.get_schedule(steps, (hw // 2) * (hw // 2), T)
        extra = {"off": {}, "off_kw": {"attn_broadcast": None}, "i2": {"attn_broadcast": 2}, "i3": {"attn_broadcast": 3}}[arm]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        den.denoise(model, img=inp["img"], timesteps=ts, img_ids=inp["img_ids"], txt_ids=inp["txt_ids"], masks=masks, masked_ref=ref, txt=inp["txt"],
                    y_vec=inp["y_vec"], **extra, **SHIPPED)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, den.last_attn_broadcast

    with torch.inference_mode():
        peak = {}
        for arm in ("off", "i2"):
            getattr(model, "_osk_ws_cache", {}).clear()
            if hasattr(model, "_osk_attn_cache"):
                object.__delattr__(model, "_osk_attn_cache")
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            torch.cuda.reset_peak_memory_stats()
            loop(arm, a.warmup_steps)
            peak[arm] = torch.cuda.max_memory_allocated()
        for arm in LOOP_ARMS:
            loop(arm, a.warmup_steps)
        ms, modes = {arm: [] for arm in LOOP_ARMS}, {}
        for _ in range(a.repeats):
            for arm in LOOP_ARMS:
                t, modes[arm] = loop(arm, a.steps)
                ms[arm].append(round(t, 2))
        med = {k: statistics.median(v) for k, v in ms.items()}
        count = lambda arm: None if modes[arm] is None else {m: modes[arm].count(m) for m in ("plain", "store", "reuse")}
        emit(dict(what="attn_broadcast_loop", model=model_name, frames=T, latent_hw=hw, L_img=L_img, L_txt=L_TXT, steps=a.steps, repeats=a.repeats,
                  range=list(sampling.ATTN_BROADCAST_RANGE), loop_ms=ms, median_ms={k: round(v, 2) for k, v in med.items()},
                  spread_ms={k: round(max(v) - min(v), 2) for k, v in ms.items()}, modes={arm: count(arm) for arm in LOOP_ARMS},
                  a_off_kw_over_off=round(med["off_kw"] / med["off"], 5), a_spread_over_median=round((max(ms["off"]) - min(ms["off"])) / med["off"], 5),
                  d_i2_over_off=round(med["i2"] / med["off"], 4), d_i3_over_off=round(med["i3"] / med["off"], 4),
                  peak_mem_off_bytes=peak["off"], peak_mem_on_bytes=peak["i2"], extra_peak_mem_bytes=peak["i2"] - peak["off"],
                  cache_bytes=cache_bytes(cfg, 3, L)))
        # ---- (b), (c): one forward at B = 3
        ac = model.attention_broadcast_begin(3, L_TXT, L_img, dev)
        sm = _time_steps(model, inp, ac, (0, 1, 2), max(a.repeats, 5))
        smed = {k: statistics.median(v) for k, v in sm.items()}
        p = PROFILE
        removed = p["attention"] + p["qkv_share_of_linears"] * p["linears"] + p["qknorm_rope"]
        emit(dict(what="attn_broadcast_step", model=model_name, B=3, L=L, step_ms=sm, median_ms={k: round(v, 3) for k, v in smed.items()},
                  spread_ms={k: round(max(v) - min(v), 3) for k, v in sm.items()}, b_store_minus_plain_ms=round(smed["store"] - smed["plain"], 3),
                  b_store_over_plain=round(smed["store"] / smed["plain"], 5), c_reuse_over_plain=round(smed["reuse"] / smed["plain"], 4),
                  profile=p, profile_removed_ms=round(removed, 1), profile_expected_reuse_over_plain=round((p["step"] - removed) / p["step"], 4),
                  expected_reuse_ms_at_measured_plain=round(smed["plain"] * (p["step"] - removed) / p["step"], 2)))
        # ---- the copy kernel alone at the loop's shapes: the single block's y row on one side, the slot on the other
        R = int(D * cfg["mlp_ratio"])
        y = torch.randn(3, L, 3 * D + R, device=dev, generator=g).to(torch.bfloat16)
        slot = torch.empty(3, L, D, dtype=torch.bfloat16, device=dev)
        v = y[:, :, 2 * D: 3 * D]
        nbytes = 4 * 3 * L * D
        for name, fn in (("store (v columns -> slot)", lambda: _C.attn_cache_copy(v, slot, None, True)),
                         ("load (slot -> v columns)", lambda: _C.attn_cache_copy(slot, v, None, False))):
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
            emit(dict(what="attn_broadcast_kernel", kernel=f"osk_attn_cache_copy_bf16 {name}", shape=[3, L, D], bytes=nbytes, median_us=round(us, 2),
                      min_us=round(min(times), 2), max_us=round(max(times), 2), tb_per_s=round(nbytes / us * 1e-6, 3)))
        # ---- the cache size as arithmetic: blocks x rows x L x D x 2 bytes
        for name, res, T_, hw_ in (("XL", "headline", T, hw), ("11B", "256 px", 33, 32), ("11B", "768 px", 33, 96)):
            c = configs.MMDIT[name]
            Ln = L_TXT + T_ * (hw_ // 2) ** 2
            emit(dict(what="attn_broadcast_cache_size", model=name, case=res, frames=T_, latent_hw=hw_, L=Ln, blocks=c["depth"] + c["depth_single_blocks"],
                      hidden=c["hidden_size"], bytes_B3=cache_bytes(c, 3, Ln), bytes_B1=cache_bytes(c, 1, Ln)))
    write_markdown(os.path.join(out_dir, "attn_broadcast.md"), _read_jsonl(jsonl))


def write_markdown(path: str, rows: list) -> None:
    lp = next((r for r in rows if r["what"] == "attn_broadcast_loop"), None)
    st = next((r for r in rows if r["what"] == "attn_broadcast_step"), None)
    gib = lambda b: f"{b / 2 ** 30:.2f} GiB"
    lines = ["# Attention broadcast: each block's attention output reused across steps", "",
             "`I2VDenoiser.denoise(attn_broadcast=interval)` (DESIGN.md section 4).  Written by `tools/attn_broadcast_time.py`; the records are in",
             "`profiles/attn_broadcast.jsonl`.  One MI355X, one process, the arms alternating; host clock around a device synchronise.", ""]
    if lp:
        m, sp = lp["median_ms"], lp["spread_ms"]
        lines += [f"Model {lp['model']}, {lp['L_img']} image + {lp['L_txt']} text tokens, CFG triple, {lp['steps']} steps of the shipped schedule, random weights, "
                  f"{lp['repeats']} repeats of each arm (median; spread = max - min); default range {tuple(lp['range'])} of the rectified-flow time "
                  "(the published [100, 800] band transcribed, NOT validated on a checkpoint).", "",
                  "| arm | loop ms (median) | spread ms | plain / store / reuse steps | over `off` |", "|---|---|---|---|---|"]
        for arm, note in (("off", "no keyword"), ("off_kw", "`attn_broadcast=None`"), ("i2", "`attn_broadcast=2`"), ("i3", "`attn_broadcast=3`")):
            c = lp["modes"][arm]
            lines.append(f"| {arm} ({note}) | {m[arm]} | {sp[arm]} | {'-' if c is None else '%d / %d / %d' % (c['plain'], c['store'], c['reuse'])} | {round(m[arm] / m['off'], 4)} |")
        lines += ["", f"(a) off: the keyword set to None against no keyword {lp['a_off_kw_over_off']}; the run-to-run spread of the `off` arm itself is "
                  f"{lp['a_spread_over_median']} of its median.  Both arms run the loop of the parent commit launch for launch (tests/test_attn_broadcast_host.py "
                  "pins the trace); the parent commit's own code was not loaded into this process.",
                  f"(d) whole loop: interval 2 {lp['d_i2_over_off']} of the off loop, interval 3 {lp['d_i3_over_off']}.",
                  f"(e) peak memory (torch.cuda.max_memory_allocated): off {lp['peak_mem_off_bytes'] / 2 ** 20:.0f} MiB, on {lp['peak_mem_on_bytes'] / 2 ** 20:.0f} MiB "
                  f"(+{lp['extra_peak_mem_bytes'] / 2 ** 20:.0f} MiB; the cache is blocks x rows x L x D x 2 bytes = {gib(lp['cache_bytes'])}).", ""]
    if st:
        m, sp, p = st["median_ms"], st["spread_ms"], st["profile"]
        lines += [f"One forward at B = {st['B']}, {st['L']} tokens (median of {len(st['step_ms']['plain'])}; spread in brackets): plain {m['plain']} ms ({sp['plain']}), "
                  f"store {m['store']} ms ({sp['store']}), reuse {m['reuse']} ms ({sp['reuse']}).", "",
                  f"(b) a store step costs {st['b_store_minus_plain_ms']} ms more than a plain one ({st['b_store_over_plain']} of it): the copies of the blocks' attention outputs.",
                  f"(c) a reuse step is {st['c_reuse_over_plain']} of a plain one.  Arithmetic from the kernel profile of the {p['step']} ms step: attention "
                  f"{p['attention']} ms + the q | k | v quarter of the {p['linears']} ms of block Linears + QK-norm / RoPE {p['qknorm_rope']} ms = {st['profile_removed_ms']} ms "
                  f"removed, i.e. {st['profile_expected_reuse_over_plain']} of the step, {st['expected_reuse_ms_at_measured_plain']} ms at the plain step measured here.  "
                  "What a reuse step still adds to that: the first LN + modulate of the single blocks stays (it feeds the MLP-up columns), one copy "
                  "of the slot per single block, and the MLP-up GEMM runs as a launch of its own.", ""]
    ks = [r for r in rows if r["what"] == "attn_broadcast_kernel"]
    if ks:
        lines += ["The copy kernel alone at the loop's shapes (20 launches each, device events):", "", "| kernel | shape | bytes | median us | TB/s |", "|---|---|---|---|---|"]
        lines += [f"| {r['kernel']} | {r['shape']} | {r['bytes']} | {r['median_us']} | {r['tb_per_s']} |" for r in ks] + [""]
    cs = [r for r in rows if r["what"] == "attn_broadcast_cache_size"]
    if cs:
        lines += ["Cache size (arithmetic, bf16): blocks x rows x L x D x 2 bytes; under sequence parallelism 1 / P of it per rank.", "",
                  "| model | case | blocks | L | D | B = 3 | B = 1 |", "|---|---|---|---|---|---|---|"]
        lines += [f"| {r['model']} | {r['case']} ({r['frames']} x {r['latent_hw']} x {r['latent_hw']} latent) | {r['blocks']} | {r['L']} | {r['hidden']} | {gib(r['bytes_B3'])} | {gib(r['bytes_B1'])} |"
                  for r in cs] + [""]
    sps = [r for r in rows if r["what"] == "attn_broadcast_sp_step"]
    if sps:
        s0 = sps[0]
        lines += ["## Under sequence parallelism: one rank's forward", "",
                  f"`tools/attn_broadcast_time.py --sharded`: model {s0['model']}, {s0['L_txt']} text + {s0['L_img']} image tokens over P = {s0['P']}, rank {s0['rank']} with "
                  f"{s0['rank_rows']} rows, exchange mode `{s0['sp_mode']}` ({'head exchange' if s0['head_exchange'] else 'all-gather'}), random weights, ONE MI355X.  The "
                  "transport is a stub whose collectives return at once and move nothing: the times are the rank's own kernels, the exchange a reuse step saves costs "
                  "nothing here either way.", "",
                  "| B | plain ms | store ms | reuse ms | store / plain | reuse / plain | stubbed exchanges plain / store / reuse | cache on this rank (single device) |",
                  "|---|---|---|---|---|---|---|---|"]
        for r in sps:
            m, ex = r["median_ms"], r["stubbed_exchanges_per_step"]
            lines.append(f"| {r['B']} | {m['plain']} | {m['store']} | {m['reuse']} | {r['store_over_plain']} | {r['reuse_over_plain']} | {ex['plain']} / {ex['store']} / {ex['reuse']} | "
                         f"{gib(r['cache_bytes'])} ({gib(r['single_device_cache_bytes'])}) |")
        lines.append("")
    lines += ["NOT measured: the output quality of reuse steps on real checkpoints (the weights here are random; the default range is a transcription, not a",
              "validated choice), and the exchange a reuse step saves on a real multi-GPU node.", ""]
    with open(path, "w") as f:
        f.write("\n".join(lines))


if __name__ == "__main__":
    main()
