#!/usr/bin/env python
"""bench.py — denoise-step latency and latent-frames/s of the MMDiT sampler on MI355X.

Workload (BASELINE.json configs[1]): XL-width MMDiT (hidden 1152, 16 heads x hd 72, 9 double + 19 single
blocks — the reference denoiser at DiT-XL/2 geometry), bf16, latent 16x64x64 (= 16x512x512
px through the 8x VAE) -> 16,384 image tokens + 512 text tokens, 30-step rectified-flow Euler sampling with
the reference's CFG triple (batch 3 per video: cond / uncond / uncond_2).  Synthetic N(0,1) latents, random
text embeddings, random-init weights (no checkpoints offline).

One "step" = one denoise step of the sampler = MMDiT forward on the CFG triple + CFG combine + Euler update.
`value` = latent frames per second for a 30-step sampling = T_lat / (30 * step_time), inputs resident in HBM.

A plain run does only what `value` needs: set up, warm up, time EXACTLY --steps steps, print the line.  Everything else the
benchmark measures (CPU baselines, the per-kernel rooflines, the batch-1 / processor / attention-dispatch side runs, the VAE,
11B and fp8 sub-objects, the rank shapes, exposed communication) runs only with --full.  --dump-outputs DIR writes what the
timed path returned after its last step as DIR/<name>.npy (float32; a fixed, seeded sample of the elements where the whole
would exceed 64 MB; the inputs are seeded: the same arguments give the same inputs in every run).

  python bench.py --gpus 1 --steps 30 --warmup 3
  python bench.py --gpus 1 --steps 30 --warmup 3 --full
  python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
         bench.py --gpus N --steps K --warmup W          (sequence parallel over the token axis, RCCL)
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
# the host driver only supports dmabuf IPC: RCCL's intra-node setup fails with hipIpcGetMemHandle otherwise
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")

import torch

SAMPLING_STEPS = 30
MFMA_BF16_PEAK_TFLOPS = 2500.0  # /opt/skills/guides/MI355X_MICROARCH.md "Peak BF16/FP16 MFMA ~2.5 PF dense"


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--model", default="XL", choices=["S", "XL", "11B"])
    ap.add_argument("--frames", type=int, default=16, help="latent frames T_lat")
    ap.add_argument("--latent-hw", type=int, default=64, help="latent height = width")
    ap.add_argument("--cfg-batch", type=int, default=3, help="3 = reference CFG triple, 1 = pure step")
    ap.add_argument("--workload", default="dit", choices=["dit", "vae"],
                    help="dit = BASELINE configs[1] (default, the headline metric); vae = configs[2]")
    ap.add_argument("--vae-frames", type=int, default=33)
    ap.add_argument("--vae-size", type=int, default=256)
    ap.add_argument("--fp8", action="store_true",
                    help="opt-in reduced precision (BASELINE configs[4]): block Linears on the fp8 (e4m3) MFMA; "
                         "never the default line -- the reference computes in bf16")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baselines")
    ap.add_argument("--no-b1", action="store_true", help="with --full: skip the extra CFG-batch-1 timing")
    ap.add_argument("--no-extra", action="store_true",
                    help="with --full: skip the `vae` (BASELINE configs[2]) and `11b` (the shipped 11B geometry) sub-objects")
    ap.add_argument("--cpu-budget-s", type=float, default=45.0)
    ap.add_argument("--full", action="store_true",
                    help="also run every side measurement (CPU baselines, rooflines, b1 / processors / attention-dispatch runs, "
                         "the vae / 11b / fp8 / rank_shapes sub-objects, exposed communication); a plain run times the headline only")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the timed path returned in its last step as DIR/<name>.npy (float32; a fixed "
                         "sample of the elements where the whole would exceed 64 MB)")
    return ap.parse_args()


def dump_outputs(out_dir, arrays, limit_bytes=64 << 20):
    """arrays: name -> tensor; written as out_dir/<name>.npy in float32.  When all of them together exceed limit_bytes, each
    is replaced by a fixed sample of its flattened elements (ascending indices drawn from a generator seeded with 0 and the
    array's size, so two runs with the same arguments sample the same positions), its share of the limit in proportion to its size;
    the size is checked before anything is written."""
    import numpy as np

    total = sum(t.numel() for t in arrays.values()) * 4
    os.makedirs(out_dir, exist_ok=True)
    for name, t in arrays.items():
        t = t.detach()
        if total > limit_bytes:
            n = t.numel()
            k = max(1, n * limit_bytes // total)
            idx = np.unique(np.random.default_rng([0, n]).integers(0, n, size=k))
            t = t.reshape(-1)[torch.from_numpy(idx).to(t.device)]
        np.save(os.path.join(out_dir, f"{name}.npy"), np.ascontiguousarray(t.float().cpu().numpy(), dtype=np.float32))


def cpu_baseline(cfg, L_img, L_txt, cfg_batch, budget_s):
    """The reference's block arithmetic timed on this host's cores on a bounded sample of the same workload: ONE double block and
    ONE single block at the full token count, batch 1; the step time is extrapolated (x depth, x CFG batch).
    kind: "reference" where the reference tree is mounted (its own DoubleStreamBlock / SingleStreamBlock through oracle/ref_loader.py)
    -- never on the GPU box, which has no /root/reference -- else "port" (oracle/mmdit_oracle.py, the pinned fp32 restatement).
    Thread count: torch's CPU operators at these sizes get SLOWER past a few dozen threads on a many-core host (round 4 timed the
    block on all 256 threads at 41 GFLOP/s while the S model on 32 reached 176), so the count is picked by a sweep of the double
    block at 1/8 of the token count and the best one is reported in `cores`.  Every second claimed here was spent: when the budget
    does not cover the single block it is NOT timed and `single_timed` says so (its time is then taken equal to the double block's,
    whose FLOP count it matches within 2 %)."""
    from oracle import mmdit_oracle as O
    from oracle import ref_loader, synth

    t_start = time.perf_counter()
    ncpu = os.cpu_count() or 1
    one = dict(cfg, depth=1, depth_single_blocks=1)
    sd = {k: torch.from_numpy(v) for k, v in synth.make_params(synth.mmdit_param_shapes(one), 0, workers=min(ncpu, 16)).items()}
    D = cfg["hidden_size"]
    hd = D // cfg["num_heads"]
    g = torch.Generator().manual_seed(0)
    img = torch.randn(1, L_img, D, generator=g)
    txt = torch.randn(1, L_txt, D, generator=g)
    vec = torch.randn(1, D, generator=g)
    ang = torch.rand(1, L_img + L_txt, hd // 2, generator=g).double()
    kind = "port"
    double = lambda i, t: O.double_block(sd, one, 0, i, t, vec, ang[:, :i.shape[1] + t.shape[1]], "interleaved")
    single = lambda x: O.single_block(sd, one, 0, x, vec, ang[:, :x.shape[1]], "interleaved")
    if ref_loader.available():
        try:
            M, _, _ = ref_loader.mmdit()
            model = M.Flux(device_map="cpu", torch_dtype=torch.float32, **one)
            model.load_state_dict(sd, strict=True)
            c, s_ = torch.cos(ang), torch.sin(ang)
            pe = torch.stack([c, -s_, s_, c], dim=-1).reshape(*ang.shape, 2, 2).float().unsqueeze(1)
            double = lambda i, t: model.double_blocks[0](i, t, vec, pe[:, :, :i.shape[1] + t.shape[1]])
            single = lambda x: model.single_blocks[0](x, vec, pe[:, :, :x.shape[1]])
            kind = "reference"
        except Exception:   # (a reference tree without the hot-path files: keep the port)
            kind = "port"
    sweep = {}
    with torch.inference_mode():
        Ls = max(256, L_img // 8)
        for n in sorted({n for n in (16, 32, 64, 128, ncpu) if n <= ncpu}):
            if time.perf_counter() - t_start > 0.25 * budget_s:
                break
            torch.set_num_threads(n)
            double(img[:, :Ls], txt)                      # warm-up of this thread count's pool
            t0 = time.perf_counter()
            double(img[:, :Ls], txt)
            sweep[n] = time.perf_counter() - t0
            if sweep[n] > 1.3 * min(sweep.values()):      # past the optimum it only gets worse (256 threads: 30 x slower) -- keep the
                break                                      # budget for the two timed blocks
        ncores = min(sweep, key=sweep.get) if sweep else min(ncpu, 32)
        torch.set_num_threads(ncores)
        t0 = time.perf_counter()
        img2, txt2 = double(img, txt)
        t_double = time.perf_counter() - t0
        single_timed = (time.perf_counter() - t_start) + 1.1 * t_double <= budget_s
        if single_timed:
            t0 = time.perf_counter()
            single(torch.cat((txt2, img2), 1))
            t_single = time.perf_counter() - t0
        else:
            t_single = t_double
    torch.set_num_threads(ncpu)
    step_s = cfg_batch * (cfg["depth"] * t_double + cfg["depth_single_blocks"] * t_single)
    return {"t_double": t_double, "t_single": t_single, "single_timed": single_timed, "step_s": step_s, "cores": ncores, "kind": kind,
            "thread_sweep_s": {str(k): round(v, 3) for k, v in sweep.items()}, "cpu_seconds": time.perf_counter() - t_start}


def cfg1_line(dev, budget_s):
    """BASELINE configs[0] (SURVEY.md section 8(d) cfg 1): ONE whole forward of the S-width MMDiT on a 1x128x128 latent
    (L_img 4096 + 512 text tokens, B = 1), the oracle (fp32, all host cores) timed whole -- no extrapolation -- beside
    the HIP path on the same weights and inputs; also reports their relative L2 difference."""
    from open_sora_amd import configs, mmdit
    from oracle import mmdit_oracle as O
    from oracle import synth

    cfg = dict(configs.MMDIT["S"])
    # this small model's operators do not scale past a few dozen threads (256 threads: 101 s per forward on the GPU
    # box, 13x slower than 8 threads): use at most 32 and report that count
    ncores = min(os.cpu_count() or 1, 32)
    torch.set_num_threads(ncores)
    sd = {k: torch.from_numpy(v) for k, v in synth.make_params(synth.mmdit_param_shapes(cfg), 0).items()}
    inp = {k: torch.from_numpy(v) for k, v in synth.mmdit_inputs(cfg, 1, 1, 64, 64, 512).items()}
    model = mmdit.Flux(device_map=dev, torch_dtype=torch.bfloat16, **cfg)
    model.load_state_dict({k: v.to(dev, torch.bfloat16) for k, v in sd.items()}, strict=True)
    ginp = {k: (v.to(dev) if k in ("img_ids", "txt_ids") else v.to(dev, torch.bfloat16)) for k, v in inp.items()}
    with torch.inference_mode():
        for _ in range(2):
            out = model(**ginp)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        n = 10
        for _ in range(n):
            out = model(**ginp)
        torch.cuda.synchronize()
        gpu_ms = (time.perf_counter() - t0) / n * 1e3
        # the same forward replayed from a hipGraph (sampling.I2VDenoiser.denoise(hip_graph=True) does this per denoise
        # step): is this small model launch-bound?  (measured: no -- same time)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out_g = model(**ginp)
        graph.replay()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            graph.replay()
        torch.cuda.synchronize()
        gpu_graph_ms = (time.perf_counter() - t0) / n * 1e3
        graph_same = bool(torch.equal(out_g, out))
        t0 = time.perf_counter()
        truth = O.forward(sd, cfg, **inp)                       # warm-up (thread pool, allocator) and the parity reference
        t_first = time.perf_counter() - t0
        times = []
        while len(times) < 3 and sum(times) + t_first < budget_s:
            t0 = time.perf_counter()
            O.forward(sd, cfg, **inp)
            times.append(time.perf_counter() - t0)
    cpu_ms = (min(times) if times else t_first) * 1e3
    o = out.float().cpu()
    rel = float((o - truth).norm() / truth.norm())
    fl = configs.flops_per_forward(cfg, 1, 4096, 512)
    return {"workload": "MMDiT-S (hidden 384, 6x64, 4+8 blocks) single forward, latent 1x128x128, L=4608, B=1",
            "cpu_ms": round(cpu_ms, 1), "cpu_timed_forwards": max(1, len(times)), "cpu_tflops": round(fl / cpu_ms / 1e9, 3),
            "cores": ncores, "kind": "port", "gpu_ms": round(gpu_ms, 3), "gpu_hipgraph_ms": round(gpu_graph_ms, 3),
            "hipgraph_bit_identical": graph_same, "rel_l2_gpu_vs_cpu_fp32": round(rel, 5)}


def vae_cpu_baseline(budget_s):
    """The oracle's CausalConv3d (fp32, thread count by a sweep) on a bounded sample: ONE 128->128 3x3x3 conv at
    9 x 128 x 128 (a slice of the encoder's first ResNet stage), scaled to the whole encode+decode by FLOPs."""
    import torch.nn.functional as F
    from oracle import vae_oracle as V

    ncpu = os.cpu_count() or 1
    g = torch.Generator().manual_seed(0)
    x = torch.randn(1, 128, 9, 128, 128, generator=g)
    sd = {"c.conv.weight": torch.randn(128, 128, 3, 3, 3, generator=g) * 0.02, "c.conv.bias": torch.zeros(128)}
    with torch.inference_mode():
        # thread count by a sweep, as the DiT leg does (torch's CPU conv does not scale to every core of a many-core host either)
        sweep, t_sweep = {}, time.perf_counter()
        for n_ in sorted({n_ for n_ in (16, 32, 64, 128, ncpu) if n_ <= ncpu}):
            torch.set_num_threads(n_)
            V.causal_conv3d(sd, "c", x[:, :, :3])  # warm-up of this pool
            t0 = time.perf_counter()
            V.causal_conv3d(sd, "c", x[:, :, :3])
            sweep[n_] = time.perf_counter() - t0
            if time.perf_counter() - t_sweep > 0.25 * budget_s or sweep[n_] > 1.3 * min(sweep.values()):
                break
        ncores = min(sweep, key=sweep.get)
        torch.set_num_threads(ncores)
        vae_cpu_baseline.sweep = {str(k_): round(v_, 3) for k_, v_ in sweep.items()}
        t0 = time.perf_counter()
        n = 0
        while True:
            V.causal_conv3d(sd, "c", x)
            n += 1
            if time.perf_counter() - t0 > min(budget_s, 20.0) or n >= 8:
                break
        dt = (time.perf_counter() - t0) / n
    torch.set_num_threads(ncpu)
    fl = 2.0 * 128 * 128 * 27 * 9 * 128 * 128
    return fl / dt, ncores, dt


def vae_line(dev, T, S, steps, warmup, cpu_budget_s, full=True, outputs=None):
    """BASELINE configs[2]: 3D-VAE (CausalConv3d) encode + decode of a [1,3,T,256,256] video, 1x MI355X.  Returns the JSON
    object (`python bench.py --workload vae` prints it as its line; the --full default line carries it as `vae`).
    full=False: the timed steps only (no per-launch events, no GroupNorm-fold run, no roofline, no CPU baseline).
    outputs: a dict that receives the decoded video of the last timed step as "video"."""
    from open_sora_amd import _C, configs, hunyuan_vae

    cfg = dict(configs.VAE["hunyuan"])

    class _A:
        pass

    args = _A()
    args.steps, args.warmup, args.no_cpu_baseline, args.cpu_budget_s = steps, warmup, cpu_budget_s is None, cpu_budget_s or 0.0
    torch.manual_seed(1234)
    model = hunyuan_vae.CausalVAE3D_HUNYUAN(device_map=dev, torch_dtype=torch.bfloat16, **cfg)
    g = torch.Generator(device=dev).manual_seed(42)
    x = (torch.randn(1, 3, T, S, S, device=dev, generator=g) * 0.5).clamp(-1, 1).to(torch.bfloat16)

    def step():
        z = model.encode(x, sample_posterior=False)
        return model.decode(z)

    with torch.inference_mode():
        for _ in range(args.warmup):
            out = step()
        _C.PROFILE_CONV = [] if full else None
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            out = step()
        torch.cuda.synchronize()
        elapsed = time.perf_counter() - t0
        prof, _C.PROFILE_CONV = _C.PROFILE_CONV, None
    assert torch.isfinite(out.float()).all() and list(out.shape) == [1, 3, 1 + 4 * ((T - 1) // 4), S, S]
    if outputs is not None:
        outputs["video"] = out
    ms = elapsed / args.steps * 1e3
    enc_f, dec_f = configs.vae_flops(cfg, T, S, S)
    res = {
        "metric": "vae_video_frames_per_sec (encode + decode; ms per encode+decode in ms_per_step)",
        "value": round(T / (ms * 1e-3), 3), "unit": "video frames/s", "n_gpus": 1, "steps": args.steps,
        "warmup": args.warmup, "ms_per_step": round(ms, 3), "higher_is_better": True, "scaling": "weak",
        "vs_baseline": None, "dtype": "bf16", "data": "synthetic",
        "config": {"workload": f"Hunyuan causal 3-D VAE (128/256/512/512, 16 latent ch) encode + decode of [1,3,{T},{S},{S}], no tiling",
                   "flops_encode": enc_f, "flops_decode": dec_f},
        "step_tflops": round((enc_f + dec_f) / (ms * 1e-3) / 1e12, 1),
        "step_mfma_frac": round((enc_f + dec_f) / (ms * 1e-3) / 1e12 / MFMA_BF16_PEAK_TFLOPS, 4),
    }
    if not full:
        del model, out
        torch.cuda.empty_cache()
        return res
    # the opt-in GroupNorm fold (hunyuan_vae.FOLD_GN: norm -> SiLU -> conv as one launch reading the un-normalised tensor) under the
    # same clock: a second, separately timed run; never part of `value`
    fold_ms = None
    if not os.environ.get("OSK_BENCH_NO_GN_FOLD"):      # (the PMC passes of tools/gpu_pmc_kernels.sh count ONE mode per process)
        was, hunyuan_vae.FOLD_GN = hunyuan_vae.FOLD_GN, True
        try:
            with torch.inference_mode():
                out_f = step()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(args.steps):
                    out_f = step()
                torch.cuda.synchronize()
                fold_ms = (time.perf_counter() - t0) / args.steps * 1e3
        finally:
            hunyuan_vae.FOLD_GN = was
        assert torch.isfinite(out_f.float()).all()
    conv_ms = sum(s.elapsed_time(e) for s, e, _ in prof) / args.steps
    ach = (enc_f + dec_f) / (conv_ms * 1e-3) / 1e12
    # HBM-side bytes of all conv launches of one step: PMC passes of this same command (tools/gpu_pmc_kernels.sh)
    traffic, traffic_src = None, None
    rec_path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "profiles", "kernel_traffic.json")
    if os.path.exists(rec_path) and (T, S) == (33, 256):
        for rec in json.load(open(rec_path)):
            if rec["kernel"].startswith(("conv256", "convsw")):   # the latest record wins
                traffic, traffic_src = rec["hbm_bytes_per_step"], rec["source"]
    res.update({
        "gn_fold": None if fold_ms is None else {"ms_per_step": round(fold_ms, 3), "what": "same model and input with hunyuan_vae.FOLD_GN = True (opt-in: GroupNorm + SiLU applied "
                    "inside the consuming sliding-window conv; 16 GB less fabric traffic per step)"},
        # all conv launches of one encode + decode: conv3d_256.hip where Cin % 128 == 0 -- the LDS sliding-window kernels
        # (convsw_kernel / convsw2_kernel) for the stride-1 3 x 3 x 3 layers incl. the fused-upsample ones, the implicit-GEMM
        # conv256x_kernel for strided / 1 x 1 x 1 layers --, conv3d_kernel (conv3d.hip) for conv_in / conv_out / the narrow layers
        "roofline": {"bound": "mfma", "kernel": "convsw_kernel + convsw2_kernel + conv256x_kernel + conv3d_kernel (by layer shape)", "achieved": round(ach, 1), "peak": MFMA_BF16_PEAK_TFLOPS,
                     "unit": "TFLOP/s", "frac": round(ach / MFMA_BF16_PEAK_TFLOPS, 4), "traffic": traffic,
                     "traffic_kind": "recorded (PMC passes of this command, see traffic_source)", "traffic_source": traffic_src,
                     "launches": len(prof) // args.steps, "total_conv_ms_per_step": round(conv_ms, 3)},
    })
    if not args.no_cpu_baseline:
        fps, ncores, dt = vae_cpu_baseline(args.cpu_budget_s)
        cpu_s = (enc_f + dec_f) / fps
        res["cpu_baseline"] = {"value": round(T / cpu_s, 5), "unit": "video frames/s", "cores": ncores, "kind": "port",
                               "thread_sweep_s": getattr(vae_cpu_baseline, "sweep", None),
                               "sample": f"oracle CausalConv3d fp32 on {ncores} host threads (best of the sweep in thread_sweep_s): one 128->128 3x3x3 conv at 9x128x128 "
                                         f"({dt:.2f} s, {fps / 1e12:.3f} TFLOP/s), encode+decode extrapolated by FLOPs = {cpu_s:.1f} s"}
    del model
    torch.cuda.empty_cache()
    return res


def _self_spawn(n: int) -> int:
    """`python bench.py --gpus N` without a launcher: re-execute this command line under torch.distributed.run with one
    rank per GPU (what the driver does for N > 1) and pass its output through."""
    import socket
    import subprocess

    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    return subprocess.call(cmd)


def main():
    args = parse()
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(_self_spawn(args.gpus))
    rank = int(os.environ.get("RANK", 0))
    world = int(os.environ.get("WORLD_SIZE", 1))
    local_rank = int(os.environ.get("LOCAL_RANK", 0))
    assert torch.cuda.is_available(), "bench.py needs MI355X GPUs (no CPU fallback for the product path)"
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    dist = None
    if world > 1:
        import torch.distributed as dist

        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("nccl", device_id=dev)
    assert world == args.gpus, f"--gpus {args.gpus} but WORLD_SIZE {world}"
    outputs = {} if args.dump_outputs else None
    if args.workload == "vae":
        assert world == 1, "the VAE workload is single-GPU (BASELINE configs[2])"
        line = vae_line(dev, args.vae_frames, args.vae_size, args.steps, args.warmup,
                        None if args.no_cpu_baseline or not args.full else args.cpu_budget_s, full=args.full, outputs=outputs)
        if outputs is not None:
            dump_outputs(args.dump_outputs, outputs)
        print(json.dumps(line), flush=True)
        return

    out = dit_line(args, dev, dist, rank, world, args.model, args.steps, args.warmup, with_b1=args.full and not args.no_b1,
                   outputs=outputs if rank == 0 else None)
    if outputs is not None and rank == 0:
        dump_outputs(args.dump_outputs, outputs)
        outputs.clear()
    if rank != 0:
        if dist is not None:
            dist.destroy_process_group()
        return
    from open_sora_amd import configs

    cfg = dict(configs.MMDIT[args.model])
    T, hw = args.frames, args.latent_hw
    L_img, L_txt = T * (hw // 2) * (hw // 2), 512
    if world == 1 and args.full and not args.no_cpu_baseline:
        cb = cpu_baseline(cfg, L_img, L_txt, 3, args.cpu_budget_s)
        td, tsg, cpu_step, ncores = cb["t_double"], cb["t_single"], cb["step_s"], cb["cores"]
        L = L_img + L_txt
        blk_flops = (8 + 4 * cfg["mlp_ratio"]) * L * cfg["hidden_size"] ** 2 + 4.0 * L * L * cfg["hidden_size"]   # one block, B = 1
        src = "the reference's own blocks (oracle/ref_loader.py)" if cb["kind"] == "reference" else "oracle fp32 (the GPU box has no reference tree: kind is 'port' there by construction)"
        single_txt = f"1 single block ({tsg:.2f} s)" if cb["single_timed"] else "the single block NOT timed (budget): taken equal to the double block"
        out["cpu_baseline"] = {
            "value": round(T / (SAMPLING_STEPS * cpu_step), 6), "unit": "latent frames/s", "cores": ncores,
            "kind": cb["kind"], "single_timed": cb["single_timed"], "cpu_seconds": round(cb["cpu_seconds"], 1),
            "thread_sweep_s": cb["thread_sweep_s"], "block_gflops": round(blk_flops / td / 1e9, 1),
            "sample": f"EXTRAPOLATED: {src} on {ncores} host threads (best of the sweep in thread_sweep_s, double block at L/8) timed on "
                      f"1 double block ({td:.2f} s) + {single_txt} at B=1, L={L}; step = x({cfg['depth']},{cfg['depth_single_blocks']}) x CFG batch 3 = {cpu_step:.1f} s "
                      f"(a whole XL step is tens of minutes of CPU; the un-extrapolated whole-forward line is cfg1)",
            "cfg1": cfg1_line(dev, args.cpu_budget_s),
        }
    if world == 1 and args.full and not args.no_extra and args.model == "XL" and not args.fp8:
        # the other two single-GPU workloads of SURVEY.md section 8(d), under the same clock as the headline: BASELINE configs[2]
        # (the causal VAE) and the geometry the reference actually ships (11B: hidden 3072, 24 x 128, 19 + 38 blocks); each with
        # its own roofline object.  Never part of `value`.
        torch.cuda.empty_cache()
        v = vae_line(dev, args.vae_frames, args.vae_size, 5, 2, None if args.no_cpu_baseline else min(args.cpu_budget_s, 20.0))
        out["vae"] = {k: v[k] for k in ("metric", "value", "unit", "ms_per_step", "steps", "warmup", "config", "step_tflops", "step_mfma_frac",
                                        "gn_fold", "roofline", "cpu_baseline") if k in v}
        b11 = dit_line(args, dev, None, 0, 1, "11B", 3, 1, with_b1=False)
        keys = ("metric", "value", "unit", "ms_per_step", "steps", "warmup", "dtype", "config", "step_tflops", "step_mfma_frac", "roofline", "roofline_gemm", "timed")
        out["11b"] = {k: b11[k] for k in keys}
        # the only shape the reference publishes a wall time for (README.md:281-287: 256 px, 129 frames, 50 steps, 60 s on one H100
        # with offload => <= 1.2 s per denoise step INCLUDING T5 / CLIP / VAE / offload traffic: an upper bound):
        # the shipped 11B model at ITS shape -- latent 33 x 28 x 36 (224 x 288 px, configs/diffusion/inference/256px.py), L = 8,316 + 512,
        # CFG triple.  Context only: other hardware, other software stack; `vs_baseline` of the headline stays null.
        r256 = dit_line(args, dev, None, 0, 1, "11B", 5, 1, with_b1=False, geom=(33, 28, 36))
        out["ref_256px_11b"] = {k: r256[k] for k in keys}
        out["ref_256px_11b"]["reference_context"] = {
            "h100_step_upper_bound_ms": 1200.0, "source": "/root/reference/README.md:281-287 (60 s / 50 steps, 1x H100, tensor parallel + offload; total includes text encoders, VAE, offload)",
            "ratio_bound_over_ours": round(1200.0 / r256["ms_per_step"], 2),
            "note": "NOT a like-for-like baseline (an upper bound on other hardware); the reference's achieved rate at this shape is >= 421 TFLOP/s (BASELINE.md section 1)"}
        # BASELINE configs[4]'s arithmetic (fp8 MFMA: block Linears + attention P.V; opt-in, outside the bf16 parity gate) on both
        # geometries, same process, same clock; roofline against the mixed bf16 / fp8 peak; rel_l2_vs_bf16 = one forward of the
        # same weights and inputs in both modes
        args.fp8 = True
        try:
            f8 = {}
            for name, st_, wu_ in (("xl", 5, 1), ("11b", 3, 1)):
                r8 = dit_line(args, dev, None, 0, 1, "XL" if name == "xl" else "11B", st_, wu_, with_b1=False)
                f8[name] = {k: r8[k] for k in keys + ("rel_l2_vs_bf16",) if k in r8}
            out["fp8"] = f8
        finally:
            args.fp8 = False
        # BASELINE configs[3] / [4] and the reference's shipped 768 px SP = 8 workload: what ONE rank of such a run computes per block
        # (attention launch with the body the model selects + the block Linears at the rank's rows), each with its roofline
        from tools import rank_shapes

        torch.cuda.empty_cache()
        out["rank_shapes"] = rank_shapes.measure(dev)
    print(json.dumps(out), flush=True)
    if dist is not None:
        dist.destroy_process_group()


def dit_line(args, dev, dist, rank, world, model_name, steps, warmup, with_b1, geom=None, outputs=None):
    """One denoise-step measurement of the product's sampler: `sampling.I2VDenoiser.denoise` (the reference's Euler loop,
    opensora/utils/sampling.py:159-226) driving MMDiTModel.forward on the CFG triple, `warmup` untimed steps, then EXACTLY
    `steps` steps between barriers.  Returns the JSON object of the line (rank 0; other ranks: None).
    args.full: also the per-launch events of the rooflines and the side measurements; without it only the timed steps run.
    outputs: a dict that receives the latents the sampler returned after the last timed step as "latents"."""
    from open_sora_amd import _C, configs, mmdit, sampling

    cfg = dict(configs.MMDIT[model_name])
    T, hw = args.frames, args.latent_hw
    hh = hw                      # latent height / width (geom: a non-square side measurement, e.g. the reference's 256 px shape)
    if geom is not None:
        T, hh, hw = geom
    L_img, L_txt = T * (hh // 2) * (hw // 2), 512
    L = L_img + L_txt
    nb = args.cfg_batch
    D, H = cfg["hidden_size"], cfg["num_heads"]
    hd = D // H

    torch.manual_seed(1234)
    model = mmdit.Flux(device_map=dev, torch_dtype=torch.bfloat16, **cfg)
    with torch.no_grad():  # random-init weights of the architecture (cond_in is zero-init in the reference)
        for n_, p_ in model.named_parameters():
            if n_.startswith("cond_in"):
                p_.normal_(0, 0.02)
    if args.fp8:
        model.enable_fp8()
    sp_mode = None
    if world > 1:
        from open_sora_amd import seqpar

        sp = seqpar.enable(model, dist.group.WORLD)   # OSK_SP_MODE=allgather|ulysses|auto (auto: head exchange for P >= 4)
        sp_mode = "all-to-all of q,k,v heads" if sp.head_parallel(H) else "all-gather of K and V^T"

    # synthetic inputs, resident in HBM before the timed region
    g = torch.Generator(device=dev).manual_seed(42)
    z = torch.randn(1, 16, T, hh, hw, device=dev, dtype=torch.bfloat16, generator=g)
    ts = sampling.get_schedule(SAMPLING_STEPS, (hh // 2) * (hw // 2), T)
    g2 = torch.Generator(device=dev).manual_seed(43)

    def sched(first, n):
        """n steps of the 30-step schedule starting at step `first` (wrapping: a benchmark may time more than one sampling)"""
        idx = [(first + i) % SAMPLING_STEPS for i in range(n)]
        return [ts[i] for i in idx] + [ts[idx[-1] + 1]]

    def barrier():
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()

    def run_denoise(x0, first, n):
        """`n` Euler steps through the product's own sampler loop (t2v: masks = 0, no reference frames); returns the latents"""
        return sampling.I2VDenoiser().denoise(
            model, img=x0.repeat(3, 1, 1), timesteps=sched(first, n), guidance=7.5, guidance_img=3.0, masks=masks, masked_ref=masked_ref,
            img_ids=img_ids, txt=txt, txt_ids=txt_ids, y_vec=y_vec)

    timed_what = "sampling.I2VDenoiser.denoise (CFG triple)"
    with torch.inference_mode():
        if nb == 3:
            txt = (torch.randn(3, L_txt, cfg["context_in_dim"], device=dev, generator=g2) * 0.2).to(torch.bfloat16)
            y_vec = torch.randn(3, cfg["vec_in_dim"], device=dev, generator=g2).to(torch.bfloat16)
            img_ids, txt_ids = sampling.prepare_ids(3, T, hh, hw, L_txt, dev, torch.bfloat16)
            masks = torch.zeros(1, 1, T, hh, hw, device=dev, dtype=torch.bfloat16)
            masked_ref = torch.zeros(1, 16, T, hh, hw, device=dev, dtype=torch.bfloat16)
            x = sampling.pack(z).contiguous()
            if warmup:
                x = run_denoise(x, 0, warmup)
            _C.PROFILE_ATTENTION = [] if rank == 0 and args.full else None
            barrier()
            t0 = time.perf_counter()
            x = run_denoise(x, warmup, steps)
            barrier()
            elapsed = time.perf_counter() - t0
            prof, _C.PROFILE_ATTENTION = _C.PROFILE_ATTENTION, None
        else:
            timed_what = f"model forward + osk_cfg_euler_bf16 at CFG batch {nb} (a private loop: the sampler's loop is the triple)"
            step, st = _plain_step(model, cfg, nb, z, ts, T, hh, hw, L_img, L_txt, dev, g2)
            for i in range(warmup):
                step(i)
            _C.PROFILE_ATTENTION = [] if rank == 0 and args.full else None
            barrier()
            t0 = time.perf_counter()
            for i in range(steps):
                step(warmup + i)
            barrier()
            elapsed = time.perf_counter() - t0
            prof, _C.PROFILE_ATTENTION = _C.PROFILE_ATTENTION, None
            x = st["x"]
        # sequence parallelism: how long the compute stream STALLED on each kind of exchange (q / k / v / o all-to-alls or the K / V^T
        # all-gathers, the final gather), from event pairs around every wait() in 2 extra steps outside the timed region
        exposed = None
        if args.full and world > 1 and nb == 3:
            sp.exposed = []
            barrier()
            run_denoise(x, 0, 2)
            barrier()
            exposed = {k_: round(v_ / 2, 3) for k_, v_ in sp.exposed_summary().items()}
            sp.exposed = None
        # roofline of the second MFMA kernel family (the Linear layers: 31 % of the XL step): HIP events around EVERY GEMM launch of
        # 2 extra steps outside the timed region (the events of 170 launches per step would perturb `value`; they do not perturb
        # a launch's own duration)
        gemm_prof = None
        if args.full and nb == 3 and world == 1:
            _C.PROFILE_GEMM = []
            torch.cuda.synchronize()
            run_denoise(x, 0, 2)
            torch.cuda.synchronize()
            gemm_prof, _C.PROFILE_GEMM = _C.PROFILE_GEMM, None
        # the attention body the timed steps ran (before any side measurement touches the QK-norm scales)
        rep = model.attention_report(world if sp_mode and "all-gather" in sp_mode else 1, L // world if world > 1 else L) if args.full else None
        # SURVEY.md section 8(d) cfg 2 asks for B = 1 (the pure step) next to the reference's CFG triple: a second, separately
        # timed run at batch 1 (reported under "b1", never part of `value`)
        b1 = None
        if nb != 1 and world == 1 and with_b1:
            step1, st1 = _plain_step(model, cfg, 1, z, ts, T, hh, hw, L_img, L_txt, dev, g2)
            n1 = max(3, min(steps, 10))
            step1(0)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(n1):
                step1(1 + i)
            torch.cuda.synchronize()
            e1 = time.perf_counter() - t0
            assert torch.isfinite(st1["x"].float()).all()
            b1 = {"cfg_batch": 1, "steps": n1, "ms_per_step": round(e1 / n1 * 1e3, 3),
                  "latent_frames_per_sec": round(T / (SAMPLING_STEPS * e1 / n1), 4),
                  "step_tflops": round(configs.flops_per_forward(cfg, 1, L_img, L_txt) / (e1 / n1) / 1e12, 1),
                  "timed": "model forward + osk_cfg_euler_bf16 at CFG batch 1 (a private loop: the sampler's loop is the triple)"}
            del step1, st1

        # The reference's own extension point (layers.py:299-303, 381-385: block.set_processor): the same 28 blocks driven ONE BY ONE
        # through HipDoubleStreamBlockProcessor / HipSingleStreamBlockProcessor with the reference forward's tensor glue around them
        # (model.py:218-229: per-block calls, torch.cat of the two streams) -- what a reference MMDiTModel with the processors
        # installed pays per forward -- beside the whole-step engine on the same inputs.  Never part of `value`.
        procs = None
        if nb == 3 and world == 1 and with_b1 and not args.fp8:
            t_vec = torch.full((3,), float(ts[0]), dtype=torch.bfloat16, device=dev)
            cond = torch.zeros(3, L_img, 68, device=dev, dtype=torch.bfloat16)
            kw = dict(img=x.repeat(3, 1, 1), img_ids=img_ids, txt=txt, txt_ids=txt_ids, timesteps=t_vec, y_vec=y_vec, cond=cond)

            def via_processors():
                ws_, vec_, rope_ = model.prepare_block_inputs(**kw)
                i_, t_ = ws_.x[:, L_txt:].clone(), ws_.x[:, :L_txt].clone()
                vb = vec_.to(torch.bfloat16)
                for blk in model.double_blocks:
                    i_, t_ = blk(i_, t_, vb, rope_)
                x_ = torch.cat((t_, i_), 1)
                for blk in model.single_blocks:
                    x_ = blk(x_, vb, rope_)
                return x_

            def engine():
                model(**kw)
                return mmdit._workspace(model, 3, L_txt, L_img, D, int(D * cfg["mlp_ratio"]), H, hd, dev).x

            def clock(fn, n):
                fn()
                torch.cuda.synchronize()
                t0_ = time.perf_counter()
                for _ in range(n):
                    r_ = fn()
                torch.cuda.synchronize()
                return (time.perf_counter() - t0_) / n * 1e3, r_

            ms_p, x_p = clock(via_processors, 3)
            x_p = x_p.float()
            ms_e, x_e = clock(engine, 3)
            procs = {"blocks": len(model.double_blocks) + len(model.single_blocks), "ms_per_forward_via_processors": round(ms_p, 3),
                     "ms_per_forward_engine": round(ms_e, 3),
                     "rel_l2_residual_stream_vs_engine": round(float((x_p - x_e.float()).norm() / x_e.float().norm()), 6),
                     "what": "per-block processor calls + the reference forward's torch.cat glue vs the whole-step engine, CFG batch 3, same inputs "
                             "(the processor path rounds vec to bf16 as the reference does; the engine keeps it in f32)"}
            del x_p, x_e

        rel8 = None
        if args.full and args.fp8 and nb == 3 and world == 1:   # one forward of the same weights and inputs in fp8 and in bf16 mode
            t_vec = torch.full((3,), float(ts[0]), dtype=torch.bfloat16, device=dev)
            cond = torch.zeros(3, L_img, 68, device=dev, dtype=torch.bfloat16)
            kw = dict(img=x.repeat(3, 1, 1), img_ids=img_ids, txt=txt, txt_ids=txt_ids, timesteps=t_vec, y_vec=y_vec, cond=cond)
            p8 = model(**kw).float()
            model.enable_fp8(False)
            p16 = model(**kw).float()
            model.enable_fp8(True)
            rel8 = float((p8 - p16).norm() / p16.norm())
            del p8, p16
        # The headline's attention body is chosen from the QK-norm scales (unit scales here).  Two side measurements under the
        # same clock (never part of `value`): (a) the same steps with the bound withheld -> the general (running-reference) body
        # a checkpoint with large scale entries would get; (b) SURVEY.md section 8(d)'s second run: scales ~U(0.5, 1.5).
        side = None
        if nb == 3 and world == 1 and with_b1 and not args.fp8:
            side = {}
            blocks = list(model.double_blocks) + list(model.single_blocks)

            def timed(n):
                _C.PROFILE_ATTENTION = []
                torch.cuda.synchronize()
                t0_ = time.perf_counter()
                xo = run_denoise(x, 0, n)
                torch.cuda.synchronize()
                e_ = time.perf_counter() - t0_
                pr, _C.PROFILE_ATTENTION = _C.PROFILE_ATTENTION, None
                return e_ / n * 1e3, sum(s_.elapsed_time(e2) for s_, e2 in pr) / len(pr), xo.float()

            plans = [b_._osk_plan for b_ in blocks]
            saved = [p_.score_bound for p_ in plans]
            for p_ in plans:
                p_.score_bound = 0.0
            mmdit.AUTO_BOUND = False                       # (a): the general body wholesale, as before round 6
            ms_g, at_g, x_gen = timed(3)
            mmdit.AUTO_BOUND = True                        # (a'): the same withheld bound, bound taken from the operands on the device
            run_denoise(x, 0, 1)
            ms_a, at_a, x_auto = timed(3)
            for p_, v_ in zip(plans, saved):
                p_.score_bound = v_
            # consistency of the two loop bodies at the timed shape (parity iii): the same 3 steps from the same
            # latents with the bound given (the body the headline ran) -- a softmax does not depend on its reference point, so the
            # two results differ by f32 rounding of the row sums, carried through 3 x 28 blocks and the bf16 residual stream
            x_fast = run_denoise(x, 0, 3).float()
            rel_fg = float((x_fast - x_gen).norm() / x_gen.norm())
            rel_fa = float((x_fast - x_auto).norm() / x_auto.norm())
            assert rel_fg < 2e-2, f"bounded (FAST) and general attention bodies disagree at the timed shape: relL2 {rel_fg:.3e}"
            assert rel_fa < 2e-2, f"host-bounded and device-bounded (auto) attention disagree at the timed shape: relL2 {rel_fa:.3e}"
            del x_fast, x_gen, x_auto
            side["general_body"] = {"steps": 3, "ms_per_step": round(ms_g, 3), "attn_avg_launch_ms": round(at_g, 4),
                                    "attention_body": _C.attention_body(hd, 1, L, 0.0), "what": "same weights, score bound withheld, auto dispatch off",
                                    "rel_l2_fast_vs_general_3_steps": round(rel_fg, 6)}
            side["auto_bound_unit_scales"] = {"steps": 3, "ms_per_step": round(ms_a, 3), "attn_avg_launch_ms": round(at_a, 4),
                                              "what": "same weights, score bound withheld: osk_rownorm2_max_bf16 on q and k + the auto-dispatched launch pair "
                                                      "(bound from the operands, per (batch, head), on the device) -- the cost of not trusting the weights",
                                              "rel_l2_fast_vs_auto_3_steps": round(rel_fa, 6)}

            def rescale(lo_, hi_, seed_):
                gs = torch.Generator(device=dev).manual_seed(seed_)
                with torch.no_grad():
                    for b_ in blocks:
                        for nrm in ([b_.img_attn.norm, b_.txt_attn.norm] if hasattr(b_, "img_attn") else [b_.norm]):
                            for prm in (nrm.query_norm.scale, nrm.key_norm.scale):
                                prm.copy_(torch.rand(prm.shape, device=dev, generator=gs) * (hi_ - lo_) + lo_)
                model.invalidate_plan()
                run_denoise(x, 0, 1)

            def device_bounds():
                """the (batch, head) bounds the LAST block's attention derived on the device (reporting only: a host read-back)"""
                ws_ = mmdit._workspace(model, 3, L_txt, L_img, D, int(D * cfg["mlp_ratio"]), H, hd, dev)
                n2 = getattr(ws_, "qk_n2", None)
                if n2 is None:
                    return None
                b_ = (n2[0] * n2[1]).sqrt().flatten().float().cpu()
                return {"min": round(float(b_.min()), 2), "max": round(float(b_.max()), 2), "pairs_on_fast_body": int((b_ <= 56.0).sum()), "pairs": int(b_.numel())}

            rescale(0.5, 1.5, 7)
            ms_s, at_s, _ = timed(3)
            rep_s = model.attention_report(1, L)
            side["qk_scales_u05_15"] = {"steps": 3, "ms_per_step": round(ms_s, 3), "attn_avg_launch_ms": round(at_s, 4),
                                        "attention_body": ", ".join(rep_s["bodies"]), "score_bound": round(rep_s["score_bound_max"], 3),
                                        "what": "QK-norm scale vectors ~U(0.5, 1.5) instead of 1 (SURVEY 8(d) second run)"}
            # scale vectors whose WEIGHT-derived bound exceeds the FAST limit (hd max|w_q| max|w_k| scale log2 e: U(0.5, 2.5) -> 76,
            # U(0.5, 4) -> 196): round 5 sent such checkpoints to the general body wholesale; now every (batch, head) whose actual
            # |q| |k| allows it runs the FAST body
            for name_, lo_, hi_, seed_ in (("qk_scales_u05_25", 0.5, 2.5, 8), ("qk_scales_u05_40", 0.5, 4.0, 9)):
                rescale(lo_, hi_, seed_)
                ms_w, at_w, xw = timed(3)
                rep_w = model.attention_report(1, L)
                assert torch.isfinite(xw).all()
                side[name_] = {"steps": 3, "ms_per_step": round(ms_w, 3), "attn_avg_launch_ms": round(at_w, 4),
                               "weight_derived_score_bound": round(rep_w["score_bound_max"], 2), "blocks_auto_dispatched": rep_w["blocks_auto_dispatched"],
                               "device_bounds_last_block": device_bounds(),
                               "what": f"QK-norm scale vectors ~U({lo_}, {hi_}): weight-derived bound above the FAST limit 56 -> bound from the operands, per (batch, head), on the device"}
                del xw

    if dist is not None:
        tmax = torch.tensor([elapsed], device=dev, dtype=torch.float64)
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
        elapsed = float(tmax.item())
    assert torch.isfinite(x.float()).all(), "non-finite latents after the timed steps"
    if outputs is not None:
        outputs["latents"] = x
    ms_per_step = elapsed / steps * 1e3
    frames_per_s = T / (SAMPLING_STEPS * ms_per_step * 1e-3)
    if rank != 0:
        return None

    # ---- roofline of the dominant kernel (attention): HIP events recorded around every launch in the timed region
    roofline = None
    if prof:
        torch.cuda.synchronize()
        durs = [s.elapsed_time(e) for s, e in prof]
        avg_ms = sum(durs) / len(durs)
        Lq = L // world
        fl = configs.attention_flops(nb, H, Lq, L, hd)  # per launch on this rank
        ach = fl / (avg_ms * 1e-3) / 1e12
        kname = _C.lib.osk_attention_kernel_name(hd, L // world).decode()
        if args.fp8 and hd in (72, 128):
            kname = f"attn_asm{hd}p8_kernel"   # fp8 mode: the fp8 P.V variant
        elif hd == 72 and L // world >= 1024 and all("FAST" in b_ for b_ in rep["bodies"]):
            kname = "attn_asm72w_kernel"       # bounded calls with >= 1024 query rows: the wide layout of the FAST body
        # HBM bytes per launch: RECORDED, not measured in this run -- PMC passes (FETCH_SIZE doubled per the gfx950 correction,
        # + WRITE_SIZE) of the same kernel at the same shape, collected by tools/gpu_final_r5.sh / tools/gpu_pmc_attn_p8.sh (PMC passes over tools/attn_only.py) and committed under profiles/
        traffic, traffic_src = None, None
        rec_path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "profiles", "attn_traffic.json")
        if os.path.exists(rec_path):
            for rec in json.load(open(rec_path)):
                if rec["kernel"] == kname and rec["shape"] == [nb, H, L, hd] and world == 1:
                    traffic, traffic_src = rec["hbm_bytes_per_launch"], rec["source"]
        peak = MFMA_BF16_PEAK_TFLOPS
        if args.fp8 and hd in (72, 128):
            # fp8 mode: QK^T (half the FLOPs) on the bf16 MFMA at 2.5 PF, P.V (the other half) on the fp8 MFMA at 5 PF:
            # the time-weighted peak for equal FLOP shares is the harmonic mean, 3.33 PF
            peak = round(2.0 / (1.0 / MFMA_BF16_PEAK_TFLOPS + 1.0 / (2 * MFMA_BF16_PEAK_TFLOPS)), 1)
        # which loop body ran is data-dependent (the FAST body needs the plans' score bound <= 56: mmdit._score_bound reads the
        # QK-norm scale vectors; freshly constructed scales are 1): report it with the bound
        body = "attn_asm%dp8_kernel<general>" % hd if (args.fp8 and hd in (72, 128)) else ", ".join(rep["bodies"])
        roofline = {"bound": "mfma", "kernel": kname, "attention_body": body,
                    "score_bound": round(rep["score_bound_max"], 3), "score_bound_limit": rep["bound_limit"],
                    "achieved": round(ach, 1),
                    "peak": peak, "unit": "TFLOP/s", "frac": round(ach / peak, 4),
                    "traffic": traffic, "traffic_kind": "recorded (PMC passes of this kernel at this shape, see traffic_source)" if traffic else "no record for this kernel / shape",
                    "traffic_source": traffic_src,
                    "algorithmic_bytes_per_launch": 4 * nb * Lq * H * hd * 2 if world == 1 else None,
                    "launches": len(durs), "avg_launch_ms": round(avg_ms, 4), "flops_per_launch": fl}
    roofline_gemm = None
    if gemm_prof:
        g_ms = sum(a_.elapsed_time(b_) for a_, b_, _ in gemm_prof) / 2
        g_fl = sum(f_ for _, _, f_ in gemm_prof) / 2
        # the block Linears only (>= 99.8 % of the GEMM FLOPs): launches of at least 1e11 FLOP -- the embedders / final layer are
        # reported with everything in `all_launches`
        blk = [(a_.elapsed_time(b_), f_) for a_, b_, f_ in gemm_prof if f_ >= 1e11]
        b_ms, b_fl = sum(t_ for t_, _ in blk) / 2, sum(f_ for _, f_ in blk) / 2
        peak_g = 2 * MFMA_BF16_PEAK_TFLOPS if args.fp8 else MFMA_BF16_PEAK_TFLOPS
        ach_g = b_fl / (b_ms * 1e-3) / 1e12
        traffic_g, traffic_g_src = None, None
        rec_path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "profiles", "kernel_traffic.json")
        if os.path.exists(rec_path) and model_name == "XL" and (T, hh, hw) == (16, 64, 64) and not args.fp8:
            for rec in json.load(open(rec_path)):
                if rec["kernel"].startswith("gemm256x"):   # the latest record wins
                    traffic_g, traffic_g_src = rec["hbm_bytes_per_step"], rec["source"]
        roofline_gemm = {"bound": "mfma", "kernel": "gemm256_kernel<fp8> (block Linears on the fp8 MFMA)" if args.fp8 else
                         "gemm256x_kernel<.,1> + gemm256x_kernel<.,2> (img + txt pairs) + gemm256x_vt_kernel (V^T written by the projection)",
                         "achieved": round(ach_g, 1), "peak": peak_g, "unit": "TFLOP/s", "frac": round(ach_g / peak_g, 4),
                         "traffic": traffic_g, "traffic_kind": "recorded per STEP (PMC passes, see traffic_source)" if traffic_g else "no record",
                         "traffic_source": traffic_g_src,
                         # per token and block, in units of D bf16 values: double = A reads 1 + 1 + 1 + 4, C writes 3 + 1 + 4 + 1, residual reads
                         # 2 = 18; single = A 1 + 5, C 7 + 1, residual 1 = 15; + every weight once
                         "algorithmic_bytes_per_step": int(nb * L * D * 2 * (cfg["depth"] * 18 + cfg["depth_single_blocks"] * 15)
                                                           + 2 * D * D * (24 * cfg["depth"] + 12 * cfg["depth_single_blocks"])),
                         "block_linear_launches_per_step": len(blk) // 2, "block_linear_ms_per_step": round(b_ms, 3), "flops_per_step": b_fl,
                         "all_launches": {"per_step": len(gemm_prof) // 2, "ms_per_step": round(g_ms, 3), "flops_per_step": g_fl},
                         "timing": "sum of HIP-event pairs around every GEMM launch, 2 steps outside the timed region"}
    step_flops = configs.flops_per_forward(cfg, nb, L_img, L_txt)
    out = {
        "metric": "latent_frames_per_sec (30-step rectified-flow sampling; denoise-step ms in ms_per_step)",
        "value": round(frames_per_s, 4), "unit": "latent frames/s", "n_gpus": world, "steps": steps,
        "warmup": warmup, "ms_per_step": round(ms_per_step, 3), "higher_is_better": True,
        "scaling": "strong", "vs_baseline": None,
        "dtype": "fp8-e4m3 block Linears (per-row scales) and attention P.V (per-head V scale); bf16 QK^T / norms / embedders" if args.fp8 else "bf16",
        "data": "synthetic",
        "config": {"workload": f"MMDiT-{model_name} (hidden {D}, {H}x{hd}, {cfg['depth']}+{cfg['depth_single_blocks']} blocks) "
                               f"denoise step, latent {T}x{hh}x{hw} ({'16x512x512 px' if (T, hh, hw) == (16, 64, 64) else f'{8 * hh}x{8 * hw} px'}), L={L} tokens, CFG batch {nb}, "
                               f"{SAMPLING_STEPS}-step Euler sampling",
                   "tokens": L, "cfg_batch": nb, "parallelism": "single GPU" if world == 1 else f"sp{world} (token axis; exchange around attention: {sp_mode})"},
        "timed": timed_what,
        "step_tflops": round(step_flops / (ms_per_step * 1e-3) / 1e12 / world, 1),
        "step_mfma_frac": round(step_flops / (ms_per_step * 1e-3) / 1e12 / world / MFMA_BF16_PEAK_TFLOPS, 4),
        "roofline": roofline,
        "roofline_gemm": roofline_gemm,
        "timing": f"time.perf_counter around EXACTLY {steps} steps between barrier + synchronize, mean (max over ranks); per-kernel figures "
                  "(roofline, roofline_gemm, rank_shapes) from HIP events on the launch stream",
    }
    if not args.full:   # a plain run records no per-launch events
        del out["roofline"], out["roofline_gemm"]
        out["timing"] = out["timing"].split("; per-kernel")[0]
    if b1 is not None:
        out["b1"] = b1
    if side:
        out["attention_dispatch"] = side
    if procs:
        out["processors"] = procs
    if rel8 is not None:
        out["rel_l2_vs_bf16"] = round(rel8, 5)
    if world > 1:
        out["rccl"] = {"world_size": dist.get_world_size(), "backend": dist.get_backend(), "exchange": sp_mode,
                       "exposed_comm_ms_per_step_rank0": exposed,
                       "exposed_comm_what": "time the compute stream stalled in wait() per exchange kind (event pairs, 2 steps outside the timed region)"}
    del model
    torch.cuda.empty_cache()
    return out


def _plain_step(model, cfg, nb, z, ts, T, hh, hw, L_img, L_txt, dev, g2):
    """forward + CFG/Euler update at an arbitrary CFG batch (the `b1` side measurement and `--cfg-batch N != 3`)"""
    from open_sora_amd import _C, sampling

    st = {"x": sampling.pack(z).contiguous()}                                # [1, L_img, 64]
    st["x_next"] = torch.empty_like(st["x"])
    txt = (torch.randn(nb, L_txt, cfg["context_in_dim"], device=dev, generator=g2) * 0.2).to(torch.bfloat16)
    y_vec = torch.randn(nb, cfg["vec_in_dim"], device=dev, generator=g2).to(torch.bfloat16)
    img_ids, txt_ids = sampling.prepare_ids(nb, T, hh, hw, L_txt, dev, torch.bfloat16)
    cond = torch.zeros(nb, L_img, 68, device=dev, dtype=torch.bfloat16)  # t2v: masks = 0, masked_ref = 0
    img3 = torch.empty(nb, L_img, 64, device=dev, dtype=torch.bfloat16)

    def step(i):
        x, x_next = st["x"], st["x_next"]
        t_curr, t_prev = ts[i % SAMPLING_STEPS], ts[i % SAMPLING_STEPS + 1]
        t_vec = torch.full((nb,), t_curr, dtype=torch.bfloat16, device=dev)
        img3.copy_(x.expand(nb, -1, -1))
        pred = model(img=img3, img_ids=img_ids, txt=txt, txt_ids=txt_ids, timesteps=t_vec, y_vec=y_vec, cond=cond)
        if nb == 3:
            _C.cfg_euler(pred, x, x_next, 7.5, 3.0, float(t_prev - t_curr))
        else:
            _C.cfg_euler(pred.expand(3, -1, -1).contiguous(), x, x_next, 1.0, 1.0, float(t_prev - t_curr))
        st["x"], st["x_next"] = x_next, x

    return step, st


if __name__ == "__main__":
    main()
