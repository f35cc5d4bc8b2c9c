"""Host side of the rectified-flow sampler around the denoiser (the caller of the hot path).

Mirrors, by name and argument meaning, the pieces of /root/reference/opensora/utils/sampling.py that sit on
either side of MMDiTModel.forward:
    get_oscillation_gs :120-133    time_shift / get_res_lin_function / get_schedule :295-332
    get_noise :335-372             pack / unpack :375-393         prepare_ids (from prepare :431-447)
    I2VDenoiser.denoise :159-226   (CFG triple, oscillating guidance, Euler update)
    DistilledDenoiser :246-279      (guidance-distilled Flux image sampling of the t2i2v pipeline)
    SamplingMethodDict :282-285    (keyed by the values of opensora/utils/inference.py:16-18, SamplingMethod)
Schedules are Python floats; tensors stay on the device; the CFG combine + Euler update is one HIP kernel
(osk_cfg_euler_bf16) instead of six bf16 elementwise launches.
"""
from __future__ import annotations

import math
import os

import torch
from torch import Tensor

from .mmdit import ops as _ops  # kernel table (HIP library; tests may swap in their CPU emulation)


def get_oscillation_gs(guidance_scale: float, i: int, force_num: int = 10) -> float:
    """sampling.py:120-133: full guidance for the first `force_num` steps and on even steps, 1.0 otherwise."""
    return guidance_scale if (i < force_num or i % 2 == 0) else 1.0


def time_shift(alpha: float, t):
    return alpha * t / (1 + (alpha - 1) * t)


def get_res_lin_function(x1: float = 256, y1: float = 1, x2: float = 4096, y2: float = 3):
    m = (y2 - y1) / (x2 - x1)
    b = y1 - m * x1
    return lambda x: m * x + b


def get_schedule(num_steps: int, image_seq_len: int, num_frames: int, shift_alpha: float | None = None,
                 base_shift: float = 1, max_shift: float = 3, shift: bool = True) -> list[float]:
    """sampling.py:307-332: linspace(1, 0, N+1) in f32, optionally shifted by alpha(seq_len) * sqrt(frames)."""
    ts = torch.linspace(1, 0, num_steps + 1)
    if shift:
        if shift_alpha is None:
            shift_alpha = get_res_lin_function(y1=base_shift, y2=max_shift)(image_seq_len)
            shift_alpha *= math.sqrt(num_frames)
        ts = time_shift(shift_alpha, ts)
    return ts.tolist()


def _ae_compression() -> int:
    return int(os.environ.get("AE_SPATIAL_COMPRESSION", 16))


def get_noise(num_samples: int, height: int, width: int, num_frames: int, device, dtype, seed: int,
              patch_size: int = 2, channel: int = 16) -> Tensor:
    """sampling.py:335-372 (device generator seeded per call)."""
    D = _ae_compression()
    gen = torch.Generator(device=device).manual_seed(seed)
    return torch.randn(num_samples, channel, num_frames, patch_size * math.ceil(height / D),
                       patch_size * math.ceil(width / D), device=device, dtype=dtype, generator=gen)


def pack(x: Tensor, patch_size: int = 2) -> Tensor:
    """'b c t (h ph) (w pw) -> b (t h w) (c ph pw)' (sampling.py:375-378)."""
    b, c, t, H, W = x.shape
    p = patch_size
    x = x.reshape(b, c, t, H // p, p, W // p, p)
    return x.permute(0, 2, 3, 5, 1, 4, 6).reshape(b, t * (H // p) * (W // p), c * p * p)


def unpack(x: Tensor, height: int, width: int, num_frames: int, patch_size: int = 2) -> Tensor:
    """'b (t h w) (c ph pw) -> b c t (h ph) (w pw)' (sampling.py:381-393)."""
    D = _ae_compression()
    h, w, p = math.ceil(height / D), math.ceil(width / D), patch_size
    b, _, cpp = x.shape
    c = cpp // (p * p)
    x = x.reshape(b, num_frames, h, w, c, p, p)
    return x.permute(0, 4, 1, 2, 5, 3, 6).reshape(b, c, num_frames, h * p, w * p)


def prepare_ids(bs: int, t: int, h: int, w: int, n_txt: int, device, dtype, patch_size: int = 2):
    """img_ids[t,h,w] = (t,h,w) in patch units, txt_ids = 0 (sampling.py:437-447,455-457)."""
    hp, wp = h // patch_size, w // patch_size
    ids = torch.zeros(t, hp, wp, 3)
    ids[..., 0] += torch.arange(t)[:, None, None]
    ids[..., 1] += torch.arange(hp)[None, :, None]
    ids[..., 2] += torch.arange(wp)[None, None, :]
    img_ids = ids.reshape(1, t * hp * wp, 3).repeat(bs, 1, 1).to(device, dtype)
    txt_ids = torch.zeros(bs, n_txt, 3, device=device, dtype=dtype)
    return img_ids, txt_ids


_SIDE_STREAMS: dict = {}   # device -> the capture stream of denoise(hip_graph=True)


def cfg_branch_counts(n_steps: int, guidance: float, guidance_img: float, text_osci: bool, image_osci: bool,
                      scale_temporal_osci: bool, dup23: bool) -> list[int]:
    """How many leading branches of the CFG triple (cond | uncond | uncond_2) each step of I2VDenoiser's loop needs for
    v = u2 + g_img (u - u2) + g_txt (c - u) (sampling.py:216), per step:
        g_img == 1.0 without a temporal ramp, or u2 == u (dup23: branches 2 and 3 get identical inputs)  ->  v = u + g_txt (c - u): 2
        ... and g_txt == 1.0 as well                                                                     ->  v = c:                 1
    The guidances are the loop's own per-step values, compared with 1.0 exactly (get_oscillation_gs returns the literal)."""
    counts = []
    for i in range(n_steps):
        text_gs = get_oscillation_gs(guidance, i) if text_osci else guidance
        image_gs = get_oscillation_gs(guidance_img, i) if image_osci else guidance_img
        ramp = image_gs > 1.0 and scale_temporal_osci
        img_one = not ramp and image_gs == 1.0
        if img_one or dup23:
            counts.append(1 if text_gs == 1.0 else 2)
        else:
            counts.append(3)
    return counts


def _branches_2_and_3_identical(masks: Tensor, masked_ref: Tensor, kwargs: dict, n: int) -> bool:
    """dup23 of cfg_branch_counts, from the tensors themselves (never from the prompts): no image condition at all -- cond3's
    third block, zeros, then equals its second -- and every tripled model input equal between blocks 2 and 3.  All comparisons
    reduce on the device into one flag: ONE host synchronisation, before step 0."""
    flags = [~masks.any(), ~masked_ref.any()]
    for v in kwargs.values():
        if torch.is_tensor(v) and v.ndim >= 1 and v.shape[0] == 3 * n:
            flags.append((v[n:2 * n] == v[2 * n:]).all())
    return bool(torch.stack(flags).all())


def _prune_default() -> bool:
    """OSK_CFG_PRUNE, read at call time (the reference's prepare_api / api_fn reach denoise() without a keyword for it)"""
    return os.environ.get("OSK_CFG_PRUNE", "") not in ("", "0")


def _window_default():
    """OSK_ATTN_WINDOW_FRAMES, read at call time like OSK_CFG_PRUNE (unset or empty: off)"""
    v = os.environ.get("OSK_ATTN_WINDOW_FRAMES", "").strip()
    return int(v) if v else None


def cond_anchor_frames(masks: Tensor) -> tuple[int, int]:
    """attn_window_anchors="cond": (head, tail) = the leading and the trailing latent frames on which `masks` ([B, 1, T, H, W],
    1 on the conditioning frames: opensora/utils/inference.py:216-351) is 1 for EVERY sample -- i2v_head (1, 0), i2v_tail (0, 1),
    i2v_loop (1, 1), text-to-video (0, 0).  A run of leading frames that reaches the last frame counts as head only.  One small
    host read."""
    on = (masks.reshape(masks.shape[0], masks.shape[1], masks.shape[2], -1) == 1).all(dim=3).all(dim=1).all(dim=0).cpu().tolist()
    T = len(on)
    head = next((i for i, v in enumerate(on) if not v), T)
    tail = next((i for i, v in enumerate(reversed(on)) if not v), T)
    return head, min(tail, T - head)


def _step_cache_default():
    """OSK_STEP_CACHE, read at call time like OSK_CFG_PRUNE: the threshold as a float (unset or empty: off)"""
    v = os.environ.get("OSK_STEP_CACHE", "").strip()
    return float(v) if v else None


def step_cache_poly(coefficients, d: float) -> float:
    """the rescaling polynomial of the step cache at d, coefficients highest power first (Horner, Python floats); None = [1, 0]"""
    r = 0.0
    for c in ([1.0, 0.0] if coefficients is None else coefficients):
        r = r * d + float(c)
    return r


def step_cache_decide(i: int, n_steps: int, d: float, acc: float, threshold: float, coefficients=None,
                      have_rows: bool = True) -> tuple[bool, float]:
    """The step cache's decision for step i of n_steps, in Python floats: (computed, acc to carry on).
    Step 0 and the last step are computed.  Any other step adds poly(d) to acc and is SKIPPED iff acc < threshold and every row
    it needs holds a residual (have_rows); otherwise it is computed.  A computed step carries acc = 0 on, a skipped one its acc.
    d = +inf (no usable distance) makes acc +inf, a NaN anywhere fails the comparison: both compute."""
    if i <= 0 or i >= n_steps - 1:
        return True, 0.0
    acc = acc + step_cache_poly(coefficients, d)
    if acc < threshold and have_rows:
        return False, acc
    return True, 0.0


def _attn_broadcast_default():
    """OSK_ATTN_BROADCAST, read at call time like OSK_CFG_PRUNE: the interval as an int (unset or empty: off)"""
    v = os.environ.get("OSK_ATTN_BROADCAST", "").strip()
    return int(v) if v else None


# The band of the published pyramid-attention-broadcast schedule, [100, 800] of 1000 diffusion timesteps, transcribed onto the
# rectified-flow time of this sampler (t runs from 1 to 0).  NOT validated on a checkpoint.
ATTN_BROADCAST_RANGE = (0.1, 0.8)


def attn_broadcast_plan(timesteps, interval, t_range=ATTN_BROADCAST_RANGE) -> list[str]:
    """The attention-broadcast mode of every step of a loop over `timesteps` (the schedule denoise() takes: N + 1 values, step i runs
    at t = timesteps[i]) -- N entries of "plain" | "store" | "reuse" (DESIGN.md section 4), from the step index and Python floats
    alone: no device value, no collective, the same list on every rank.
    Step 0 and the last step are plain; so is every step whose t lies outside [lo, hi] (both ends inclusive).  The steps inside
    cycle through one computed step followed by interval - 1 reuse steps; leaving the range ends the cycle.  A computed step is
    "store" iff the step after it is "reuse", else "plain".  interval <= 1: all plain."""
    n = len(timesteps) - 1
    lo, hi = (float(v) for v in t_range)
    interval = int(interval)
    modes = ["plain"] * max(n, 0)
    if interval <= 1:
        return modes
    pos = 0
    for i in range(n):
        if not (0 < i < n - 1 and lo <= float(timesteps[i]) <= hi):
            pos = 0
            continue
        modes[i] = "reuse" if pos else "computed"
        pos = (pos + 1) % interval
    return [("store" if i + 1 < n and modes[i + 1] == "reuse" else "plain") if m == "computed" else m for i, m in enumerate(modes)]


def attn_broadcast_effective(plan, counts, n: int = 1) -> list[str]:
    """what the steps of a loop actually run: the plan, with the cache's per-row entries followed on the host.  Step i runs the
    counts[i] * n leading rows.  A computed step ("plain" or "store") drops every entry -- an entry is only ever reused inside the
    cycle that stored it -- and a "store" step then leaves one for each of its rows; a "reuse" step that needs a row without an
    entry (a pruned loop whose step runs more branches than the cycle's store did) becomes a "store" step.  Static, like the plan."""
    have = [False] * (max(counts, default=0) * n)
    out = []
    for mode, nb in zip(plan, counts):
        m = nb * n
        if mode == "reuse" and not all(have[:m]):
            mode = "store"
        if mode != "reuse":
            have = [False] * len(have)
        if mode == "store":
            have[:m] = [True] * m
        out.append(mode)
    return out


class I2VDenoiser:
    """sampling.py:158-245.  `denoise(model, img=..., timesteps=[...], guidance=..., guidance_img=..., masks=...,
    masked_ref=..., img_ids=..., txt=..., txt_ids=..., y_vec=..., [text_osci, image_osci, scale_temporal_osci,
    patch_size, sigma_min])` with img/txt/... already tripled (cond | uncond | uncond_2).

    Not in the reference: `hip_graph=True` replays the model forward of steps 1.. from a hipGraph captured after step 0
    (every entry point of the library is capturable: no allocation, no synchronisation; the per-step inputs -- the
    latent triple and the timestep vector -- live in fixed buffers).  Same results bit for bit.  Measured on this host:
    no gain at either end -- the XL step's ~540 launches hide behind 150 ms of kernels, and even the S model's 2.6 ms
    forward replays in the same 2.6 ms (`bench.py`: cpu_baseline.cfg1.gpu_hipgraph_ms) -- so it is off by default and
    meant for hosts whose Python dispatch is slower than the GPU.

    Not in the reference either: `cfg_prune=True` (default: the environment variable OSK_CFG_PRUNE, read at call time) runs at every
    step only the branches of the triple that step's guidance uses (cfg_branch_counts): one where both guidances are 1.0 -- 20 of
    the 50 steps of the shipped oscillating schedule -- and two throughout when there is no image condition and the two negative
    prompts are the same tensor rows (text-to-video).  The skipped branches cancel in sampling.py:216 exactly in real arithmetic; in
    bf16 the result differs from the triple's by rounding only (tests/test_gpu_cfg_prune.py holds it to the project's parity rule).
    Off, the loop is the one above, launch for launch.  With hip_graph, one graph per branch count in use.  `last_branch_counts`
    holds the counts of the last run.  Cost: one activation workspace set per batch size in use instead of one.

    `attn_window_frames=W` (default: OSK_ATTN_WINDOW_FRAMES, read at call time; unset = off): opt-in frame-window attention for
    this loop -- MMDiTModel.set_attention_window(W, frame_tokens) with frame_tokens from masked_ref's h, w and patch_size, also
    under hip_graph and cfg_prune; the model's previous setting is restored afterwards.  Results differ from the reference's
    (every query sees every key) by what the dropped keys carried; output quality on real checkpoints is not measured.
    `attn_window_anchors=None | (head, tail) | "cond"` (with attn_window_frames; without it: ValueError): latent frames every query
    keeps attending to -- "cond" takes them from `masks` (cond_anchor_frames: the reference frames the loop conditions on), one
    small host read before step 0.  Composes with hip_graph, cfg_prune and step_cache as the window does.

    `step_cache=threshold` (default: OSK_STEP_CACHE, read at call time; unset = off) with `step_cache_coefficients=None`: opt-in
    step cache of the TeaCache kind.  Every step runs the model's head and measures how far block 0's modulated image input of
    the conditional rows moved since the previous step (relative L1, osk_step_delta_bf16); while the accumulated, polynomial-
    rescaled movement stays under the threshold (step_cache_decide) the block stack is skipped and the last computed residual
    of each row is added to the embedded latents instead (DESIGN.md section 4 states the rule).  Works with cfg_prune (residuals
    are kept per row of the triple) and attn_window_frames; refused with hip_graph and for models without the head / blocks /
    tail split.  One 8-byte read back per step.  `last_step_cache` holds (d, acc, computed) per step of the last run (None when
    off).  Under sequence parallelism (seqpar.enable) every rank measures the distance over its own image rows, the P pairs of
    sums travel in one 8-byte all-gather per step and are added in rank order on every rank (osk_step_sums_combine_f32): the
    same bits, hence the same decisions and the same `last_step_cache` on all ranks, with no broadcast; the cache's buffers are
    cut to the rank's rows (1 / P of the memory per rank).  All exchange modes, ragged splits, kv_chunks, fp8 / qk8 and cfg_prune
    are accepted; still refused there: a frame window together with the step cache, and an sp object without SeqPar.step_cache.
    The exchange of the sums on a multi-GPU node is not measured.
    No calibrated polynomial ships (default: the identity), and neither the skip rate nor the
    output quality on real checkpoints is measured: a skipped step's result DIFFERS from the reference's.

    `attn_broadcast=interval` (default: OSK_ATTN_BROADCAST, read at call time; unset or <= 1 = off) with
    `attn_broadcast_range=(lo, hi)`: opt-in attention broadcast of the pyramid-attention-broadcast kind.  Inside the range of the
    rectified-flow time every interval-th step computes its attention and stores each block's attention output
    (osk_attn_cache_copy_bf16 into a slot per block); the interval - 1 steps behind it run their own modulation, projections and MLPs
    but take the attention output from the slot: no q | k | v projection, QK-norm / RoPE or attention launch, and under sequence
    parallelism no K / V exchange (attn_broadcast_plan states the schedule, DESIGN.md section 4 the rule).  The schedule depends on
    the step index alone: no read back, no collective, and with hip_graph one graph per (batch size, mode) in use.  Composes
    with cfg_prune (entries are kept per row; a reuse step that needs a row without one computes and stores instead:
    attn_broadcast_effective), attn_window_frames / anchors, fp8 / qk8, sequence parallelism and step_cache (a step the step
    cache skips launches no block: it neither stores nor reuses).  `last_attn_broadcast` holds the mode each step of the last run
    took (None when off).  Memory: blocks x rows x L x D x 2 bytes (under sequence parallelism 1 / P of it per rank).  The
    default range (0.1, 0.8) is the published method's [100, 800]-of-1000 band transcribed onto this schedule; it is NOT
    validated on a checkpoint, and the output quality on real checkpoints is not measured: a reuse step's result DIFFERS from the
    reference's.  Refused for models without the head / blocks / tail split."""

    def denoise(self, model, **kwargs) -> Tensor:
        img = kwargs.pop("img")
        timesteps = kwargs.pop("timesteps")
        guidance = kwargs.pop("guidance")
        guidance_img = kwargs.pop("guidance_img")
        masks = kwargs.pop("masks")
        masked_ref = kwargs.pop("masked_ref")
        kwargs.pop("sigma_min", None)
        text_osci = kwargs.pop("text_osci", False)
        image_osci = kwargs.pop("image_osci", False)
        scale_temporal_osci = kwargs.pop("scale_temporal_osci", False)
        patch_size = kwargs.pop("patch_size", 2)
        hip_graph = bool(kwargs.pop("hip_graph", False))
        cfg_prune = kwargs.pop("cfg_prune", None)
        cfg_prune = _prune_default() if cfg_prune is None else bool(cfg_prune)
        attn_window_frames = kwargs.pop("attn_window_frames", "env")
        if isinstance(attn_window_frames, str) and attn_window_frames == "env":
            attn_window_frames = _window_default()
        anchors = kwargs.pop("attn_window_anchors", None)
        if anchors is not None and attn_window_frames is None:
            raise ValueError("attn_window_anchors needs attn_window_frames: anchor frames belong to frame-window attention")
        step_cache = kwargs.pop("step_cache", "env")
        if isinstance(step_cache, str) and step_cache == "env":
            step_cache = _step_cache_default()
        coefficients = kwargs.pop("step_cache_coefficients", None)
        attn_broadcast = kwargs.pop("attn_broadcast", "env")
        if isinstance(attn_broadcast, str) and attn_broadcast == "env":
            attn_broadcast = _attn_broadcast_default()
        ab_range = kwargs.pop("attn_broadcast_range", None)
        self.last_attn_broadcast = None
        if attn_broadcast is not None:
            attn_broadcast = int(attn_broadcast)
            ab_range = ATTN_BROADCAST_RANGE if ab_range is None else tuple(float(v) for v in ab_range)
            if len(ab_range) != 2 or not ab_range[0] <= ab_range[1]:
                raise ValueError(f"attn_broadcast_range: (lo, hi) with lo <= hi expected; got {ab_range}")
            if not all(hasattr(model, a) for a in ("attention_broadcast_begin", "forward_ckpt", "step_run")):
                raise ValueError("attn_broadcast needs a model with the head / blocks / tail split and a cache slot per block "
                                 f"(open_sora_amd.mmdit.MMDiTModel); {type(model).__name__} has none")
            if attn_broadcast <= 1:
                attn_broadcast = None                    # every step plain: the loop from before, launch for launch
        self.last_step_cache = None
        if step_cache is not None:
            step_cache = float(step_cache)
            coefficients = None if coefficients is None else [float(c) for c in coefficients]
            # out of scope for this change, refused before anything runs
            if not all(hasattr(model, a) for a in ("step_cache_begin", "step_head", "step_run", "step_skip", "step_distance")):
                raise ValueError("step_cache needs a model with the head / blocks / tail split (open_sora_amd.mmdit.MMDiTModel); "
                                 f"{type(model).__name__} has none")
            sp = getattr(model, "_sp", None)
            if sp is not None and not getattr(sp, "step_cache", False):      # (an sp object from before the sharded step cache)
                raise ValueError("step_cache does not run under sequence parallelism (every rank would have to take the same decision)")
            if hip_graph:
                raise ValueError("step_cache and hip_graph=True do not combine: the decision sits on the host between the head and the blocks")
            if sp is not None and (attn_window_frames is not None or getattr(model, "_attn_window", None) is not None):
                raise ValueError("step_cache: frame-window attention, sequence parallelism and the step cache do not run together (any two "
                                 "of them do); leave attn_window_frames off, run without seqpar.enable or leave step_cache off")
        if attn_window_frames is not None:
            # opt-in frame-window attention for this loop (MMDiTModel.set_attention_window): a latent frame is (h / patch) * (w / patch)
            # tokens of the packed sequence; the model's previous setting comes back afterwards, whatever the loop does
            if not hasattr(model, "set_attention_window"):
                raise ValueError("attn_window_frames needs a model with set_attention_window (open_sora_amd.mmdit.MMDiTModel)")
            ps = patch_size
            previous = getattr(model, "_attn_window", None)
            previous_anchors = getattr(model, "_attn_anchors", None)
            if isinstance(anchors, str) and anchors == "cond":
                anchors = cond_anchor_frames(masks)
            # (no anchors asked for: the call from before, in which the model reads OSK_ATTN_WINDOW_ANCHORS)
            kw = {} if anchors is None else {"anchors": tuple(anchors)}
            model.set_attention_window(int(attn_window_frames), (masked_ref.shape[-2] // ps) * (masked_ref.shape[-1] // ps), **kw)
            try:
                return self.denoise(model, img=img, timesteps=timesteps, guidance=guidance, guidance_img=guidance_img, masks=masks,
                                    masked_ref=masked_ref, text_osci=text_osci, image_osci=image_osci,
                                    scale_temporal_osci=scale_temporal_osci, patch_size=patch_size, hip_graph=hip_graph,
                                    cfg_prune=cfg_prune, attn_window_frames=None, step_cache=step_cache,
                                    step_cache_coefficients=coefficients, attn_broadcast=attn_broadcast, attn_broadcast_range=ab_range,
                                    **kwargs)
            finally:
                model.set_attention_window(*(previous if previous is not None else (None,)),
                                           **({"anchors": previous_anchors} if previous is not None and hasattr(model, "_attn_anchors") else {}))

        n3 = img.shape[0]
        n = n3 // 3
        counts = [3] * (len(timesteps) - 1)
        if cfg_prune:
            counts = cfg_branch_counts(len(timesteps) - 1, guidance, guidance_img, text_osci, image_osci, scale_temporal_osci,
                                       _branches_2_and_3_identical(masks, masked_ref, kwargs, n))
        self.last_branch_counts = counts
        loop = self._loop_pruned if cfg_prune else self._loop
        tail = (counts,) if cfg_prune else ()
        dev, dt = img.device, img.dtype
        guidance_vec = torch.full((n3,), guidance, device=dev, dtype=dt)
        b, c, t, w_, h_ = masked_ref.size()
        cond = pack(torch.cat((masks, masked_ref), dim=1), patch_size=patch_size)
        cond3 = torch.cat([cond, cond, torch.zeros_like(cond)], dim=0)  # 3rd branch drops the image condition
        # private state (the ping-pong below must not write into the caller's tensor), kept in bf16 -- the dtype the
        # update kernel computes in and the reference samples in (configs/diffusion/inference/256px.py:4); a model in
        # another dtype is fed / read through casts at this boundary
        x = img[:n].to(torch.bfloat16, copy=True).contiguous()
        x_next = torch.empty_like(x)
        img3 = torch.empty(n3, *x.shape[1:], device=dev, dtype=dt)
        t_vec = torch.empty(n3, dtype=dt, device=dev)
        ab = {}
        if attn_broadcast is not None:
            # the static schedule of this loop; the loops below follow the cache's entries from it
            self.last_attn_broadcast = []
            ab = {"ab": (attn_broadcast_plan(timesteps, attn_broadcast, ab_range), self.last_attn_broadcast)}
        if step_cache is not None:
            self.last_step_cache = []
            return self._loop_step_cache(model, kwargs, x, x_next, img3, t_vec, cond3, guidance_vec, timesteps, guidance, guidance_img,
                                         text_osci, image_osci, scale_temporal_osci, patch_size, b, c, t, h_, w_, dev, counts, cfg_prune,
                                         step_cache, coefficients, self.last_step_cache, **ab).to(dt)
        if ab:
            loop, tail = self._loop_attn_broadcast, (counts, cfg_prune) + ab["ab"]
        graph, pred = None, None
        if hip_graph:
            # capture needs a non-default stream, and the model's workspaces are keyed on the stream: run the WHOLE loop (the
            # eager step 0 as well) on one side stream, so capture re-uses step 0's workspaces instead of allocating a second
            # set from the graph's private pool that would stay pinned for the model's lifetime
            # ONE side stream per device for the lifetime of the process (the workspace key contains the stream handle: a fresh
            # stream per call would allocate a fresh activation workspace set per sampling run -- ADVICE r3)
            side = _SIDE_STREAMS.get(str(dev))
            if side is None:
                side = _SIDE_STREAMS[str(dev)] = torch.cuda.Stream(dev)
            side.wait_stream(torch.cuda.current_stream(dev))
            with torch.cuda.stream(side):
                out = loop(model, kwargs, x, x_next, img3, t_vec, cond3, guidance_vec, timesteps, guidance, guidance_img,
                           text_osci, image_osci, scale_temporal_osci, patch_size, b, c, t, h_, w_, dev, True, side, *tail)
            torch.cuda.current_stream(dev).wait_stream(side)
            return out.to(dt)
        return loop(model, kwargs, x, x_next, img3, t_vec, cond3, guidance_vec, timesteps, guidance, guidance_img, text_osci,
                    image_osci, scale_temporal_osci, patch_size, b, c, t, h_, w_, dev, False, None, *tail).to(dt)

    @staticmethod
    def _loop(model, kwargs, x, x_next, img3, t_vec, cond3, guidance_vec, timesteps, guidance, guidance_img, text_osci, image_osci,
              scale_temporal_osci, patch_size, b, c, t, h_, w_, dev, hip_graph, side):
        graph, pred = None, None
        for i, (t_curr, t_prev) in enumerate(zip(timesteps[:-1], timesteps[1:])):
            t_vec.fill_(t_curr)
            if _ops().copy_rows_ok(x, img3[:x.shape[0]]):
                # the CFG triple's input = the latents three times over (sampling.py:196-201): one broadcast launch for one sample
                for j in ([None] if x.shape[0] == 1 else range(3)):
                    _ops().copy_rows(x, img3 if j is None else img3[j * x.shape[0]:(j + 1) * x.shape[0]])
            else:
                img3.view(3, *x.shape).copy_(x.unsqueeze(0).expand(3, *x.shape))
            if graph is not None:
                graph.replay()                    # writes the captured `pred`
            else:
                pred = model(img=img3, **kwargs, cond=cond3, timesteps=t_vec, guidance=guidance_vec)
                if hip_graph and i == 0 and len(timesteps) > 2:
                    # step 0 ran eagerly (it built the plans and workspaces); capture the same call for the rest
                    graph = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(graph, stream=side):
                        pred_g = model(img=img3, **kwargs, cond=cond3, timesteps=t_vec, guidance=guidance_vec)
            text_gs = get_oscillation_gs(guidance, i) if text_osci else guidance
            image_gs = get_oscillation_gs(guidance_img, i) if image_osci else guidance_img
            gvec = None
            if image_gs > 1.0 and scale_temporal_osci:
                upper = torch.linspace(image_gs, 1.0, len(timesteps))[i]
                ramp = torch.linspace(1.0, float(upper), t)[None, None, :, None, None].repeat(b, c, 1, h_, w_)
                gvec = pack(ramp, patch_size=patch_size).to(dev, torch.float32).contiguous()
                image_gs = 1.0
            _ops().cfg_euler(pred.to(torch.bfloat16).contiguous(), x, x_next, float(text_gs), float(image_gs),
                             float(t_prev - t_curr), gvec)
            x, x_next = x_next, x
            if graph is not None:
                pred = pred_g                     # from now on the forward's output is the captured tensor
        return x

    @staticmethod
    def _loop_pruned(model, kwargs, x, x_next, img3, t_vec, cond3, guidance_vec, timesteps, guidance, guidance_img, text_osci,
                     image_osci, scale_temporal_osci, patch_size, b, c, t, h_, w_, dev, hip_graph, side, counts):
        """_loop with cfg_prune: step i runs the model on the counts[i] leading branches only (cfg_branch_counts) and combines them
        with osk_cfg_euler_nb_bf16.  The kept branches are a prefix of every tripled tensor, so a branch count's inputs are views of
        the triple's buffers made ONCE: the same tensor objects every step (the model's position-embedding memo keeps hitting), at
        fixed addresses (a captured graph reads them)."""
        n = x.shape[0]
        inputs = {}    # branch count -> the model's keyword arguments for it
        graphs = {}    # branch count -> (hipGraph of the forward at that batch, its output tensor)
        for i, (t_curr, t_prev) in enumerate(zip(timesteps[:-1], timesteps[1:])):
            nb = counts[i]
            kw = inputs.get(nb)
            if kw is None:
                m = nb * n
                kw = inputs[nb] = {k: (v[:m] if torch.is_tensor(v) and v.ndim >= 1 and v.shape[0] == 3 * n else v) for k, v in kwargs.items()}
                kw.update(img=img3[:m], cond=cond3[:m], timesteps=t_vec[:m], guidance=guidance_vec[:m])
            t_vec.fill_(t_curr)
            dst = kw["img"]
            if _ops().copy_rows_ok(x, dst[:n]):
                for j in ([None] if n == 1 else range(nb)):
                    _ops().copy_rows(x, dst if j is None else dst[j * n:(j + 1) * n])
            else:
                dst.view(nb, *x.shape).copy_(x.unsqueeze(0).expand(nb, *x.shape))
            if nb in graphs:
                graphs[nb][0].replay()            # writes the captured prediction of this branch count
                pred = graphs[nb][1]
            else:
                pred = model(**kw)
                if hip_graph and nb in counts[i + 1:]:
                    # as step 0 of _loop: the first step of a branch count ran eagerly (it built that batch size's workspaces), the
                    # same call is captured for the later ones -- one graph per count in use, all on the one side stream, no
                    # parallel capture branches.  A loop uses at most three batch sizes and mmdit._workspace keeps four geometries
                    # per model, least recently INSERTED first out (a replay does not touch the cache): at most two sets are
                    # inserted behind the first one during a loop, so no set a live graph replays into is evicted.  The same
                    # count holds for seqpar's exchange buffers (SeqPar.MAX_GEOMETRIES = 4, one set per batch size and forward).
                    g = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(g, stream=side):
                        pred_g = model(**kw)
                    graphs[nb] = (g, pred_g)
            text_gs = get_oscillation_gs(guidance, i) if text_osci else guidance
            image_gs = get_oscillation_gs(guidance_img, i) if image_osci else guidance_img
            gvec = None
            if nb == 3 and image_gs > 1.0 and scale_temporal_osci:
                upper = torch.linspace(image_gs, 1.0, len(timesteps))[i]
                ramp = torch.linspace(1.0, float(upper), t)[None, None, :, None, None].repeat(b, c, 1, h_, w_)
                gvec = pack(ramp, patch_size=patch_size).to(dev, torch.float32).contiguous()
                image_gs = 1.0
            _ops().cfg_euler_nb(pred.to(torch.bfloat16).contiguous(), nb, x, x_next, float(text_gs), float(image_gs),
                                float(t_prev - t_curr), gvec)
            x, x_next = x_next, x
        return x

    @staticmethod
    def _loop_step_cache(model, kwargs, x, x_next, img3, t_vec, cond3, guidance_vec, timesteps, guidance, guidance_img, text_osci,
                         image_osci, scale_temporal_osci, patch_size, b, c, t, h_, w_, dev, counts, pruned, threshold, coefficients,
                         record, ab=None):
        """_loop (pruned: _loop_pruned) with the step cache: the model's forward is driven in its three parts.  Every step runs the
        head on its counts[i] leading branches and the distance of the conditional rows; step_cache_decide then picks the block
        stack (step_run: the rows' residuals are stored) or the stored residuals (step_skip).  The inputs, the combine kernel and
        their order are those of the loop it stands for, so a run that computes every step gives that loop's bits.
        ab = (plan, record) with attention broadcast on as well: the plan is indexed by step; a computed step runs its blocks in the
        plan's mode (a reuse step that lacks an entry stores instead), a skipped step launches no block and touches no entry --
        except that a skipped step the plan wanted computed drops the entries, so the reuse steps behind it compute."""
        n = x.shape[0]
        n_steps = len(timesteps) - 1
        ac = None if ab is None else model.attention_broadcast_begin(max(counts, default=3) * n, kwargs["txt"].shape[1], img3.shape[1], dev)
        # (a sharded model cuts the buffers to its rank's rows and needs the text length for that; every rank then measures its share
        # of the distance and all of them read the same combined sums, so the decisions below are the same on every rank)
        sharded = {} if getattr(model, "_sp", None) is None else {"L_txt": kwargs["txt"].shape[1]}
        sc = model.step_cache_begin(n, max(counts, default=3) * n, img3.shape[1], dev, **sharded)
        inputs = {}    # branch count -> the model's keyword arguments for it (views made once, as in _loop_pruned)
        acc = 0.0
        for i, (t_curr, t_prev) in enumerate(zip(timesteps[:-1], timesteps[1:])):
            nb = counts[i]
            m = nb * n
            kw = inputs.get(nb)
            if kw is None:
                kw = inputs[nb] = {k: (v[:m] if torch.is_tensor(v) and v.ndim >= 1 and v.shape[0] == 3 * n else v) for k, v in kwargs.items()}
                kw.update(img=img3[:m], cond=cond3[:m], timesteps=t_vec[:m], guidance=guidance_vec[:m])
            t_vec.fill_(t_curr)
            dst = kw["img"]
            if _ops().copy_rows_ok(x, dst[:n]):
                for j in ([None] if n == 1 else range(nb)):
                    _ops().copy_rows(x, dst if j is None else dst[j * n:(j + 1) * n])
            else:
                dst.view(nb, *x.shape).copy_(x.unsqueeze(0).expand(nb, *x.shape))
            st = model.step_head(sc, **kw)
            d = math.inf if i == 0 else model.step_distance(sc)       # the one host synchronisation of a step
            computed, acc = step_cache_decide(i, n_steps, d, acc, threshold, coefficients, all(sc.have[:m]))
            if ab is None:
                pred = model.step_run(sc, st) if computed else model.step_skip(sc, st)
            else:
                mode = ab[0][i]
                if computed and mode == "reuse" and not all(ac.have[:m]):
                    mode = "store"
                if mode != "reuse":
                    ac.clear()
                pred = (model.step_run(sc, st, None if mode == "plain" else (ac, mode, tuple(range(m)))) if computed else
                        model.step_skip(sc, st))
                ab[1].append(mode if computed else "skipped")
            record.append((d, acc, computed))
            text_gs = get_oscillation_gs(guidance, i) if text_osci else guidance
            image_gs = get_oscillation_gs(guidance_img, i) if image_osci else guidance_img
            gvec = None
            if nb == 3 and image_gs > 1.0 and scale_temporal_osci:
                upper = torch.linspace(image_gs, 1.0, len(timesteps))[i]
                ramp = torch.linspace(1.0, float(upper), t)[None, None, :, None, None].repeat(b, c, 1, h_, w_)
                gvec = pack(ramp, patch_size=patch_size).to(dev, torch.float32).contiguous()
                image_gs = 1.0
            pred = pred.to(torch.bfloat16).contiguous()
            if pruned:
                _ops().cfg_euler_nb(pred, nb, x, x_next, float(text_gs), float(image_gs), float(t_prev - t_curr), gvec)
            else:
                _ops().cfg_euler(pred, x, x_next, float(text_gs), float(image_gs), float(t_prev - t_curr), gvec)
            x, x_next = x_next, x
        return x

    @staticmethod
    def _loop_attn_broadcast(model, kwargs, x, x_next, img3, t_vec, cond3, guidance_vec, timesteps, guidance, guidance_img, text_osci,
                             image_osci, scale_temporal_osci, patch_size, b, c, t, h_, w_, dev, hip_graph, side, counts, pruned, plan,
                             record):
        """_loop (pruned: _loop_pruned) with attention broadcast: step i runs the model on its counts[i] leading branches in the mode
        attn_broadcast_effective gives it -- "plain": the forward as ever; "store" / "reuse": forward_ckpt(attn_cache=...) on the
        loop's cache, rows = the leading rows of the triple.  The inputs, the combine kernel and their order are those of the loop
        it stands for.  hip_graph: as in _loop_pruned, the first step of every (branch count, mode) runs eagerly and is captured
        for the later ones -- the modes are known up front, the row maps and the cache never move."""
        n = x.shape[0]
        modes = attn_broadcast_effective(plan, counts, n)
        ac = model.attention_broadcast_begin(max(counts, default=3) * n, kwargs["txt"].shape[1], img3.shape[1], dev)
        inputs = {}    # branch count -> the model's keyword arguments for it
        graphs = {}    # (branch count, mode) -> (hipGraph of the forward, its output tensor)
        keys = list(zip(counts, modes))
        for i, (t_curr, t_prev) in enumerate(zip(timesteps[:-1], timesteps[1:])):
            nb, mode = keys[i]
            m = nb * n
            kw = inputs.get(nb)
            if kw is None:
                kw = inputs[nb] = {k: (v[:m] if torch.is_tensor(v) and v.ndim >= 1 and v.shape[0] == 3 * n else v) for k, v in kwargs.items()}
                kw.update(img=img3[:m], cond=cond3[:m], timesteps=t_vec[:m], guidance=guidance_vec[:m])
            t_vec.fill_(t_curr)
            dst = kw["img"]
            if _ops().copy_rows_ok(x, dst[:n]):
                for j in ([None] if n == 1 else range(nb)):
                    _ops().copy_rows(x, dst if j is None else dst[j * n:(j + 1) * n])
            else:
                dst.view(nb, *x.shape).copy_(x.unsqueeze(0).expand(nb, *x.shape))
            rows = tuple(range(m))
            if mode != "reuse":
                ac.clear()
            if (nb, mode) in graphs:
                graphs[(nb, mode)][0].replay()
                pred = graphs[(nb, mode)][1]
                if mode == "store":
                    ac.mark(rows)                 # (an eager store forward marks its rows itself)
            else:
                extra = {} if mode == "plain" else {"attn_cache": (ac, mode, rows)}
                pred = model(**kw, **extra)
                if hip_graph and (nb, mode) in keys[i + 1:]:
                    g = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(g, stream=side):
                        pred_g = model(**kw, **extra)
                    graphs[(nb, mode)] = (g, pred_g)
            record.append(mode)
            text_gs = get_oscillation_gs(guidance, i) if text_osci else guidance
            image_gs = get_oscillation_gs(guidance_img, i) if image_osci else guidance_img
            gvec = None
            if nb == 3 and image_gs > 1.0 and scale_temporal_osci:
                upper = torch.linspace(image_gs, 1.0, len(timesteps))[i]
                ramp = torch.linspace(1.0, float(upper), t)[None, None, :, None, None].repeat(b, c, 1, h_, w_)
                gvec = pack(ramp, patch_size=patch_size).to(dev, torch.float32).contiguous()
                image_gs = 1.0
            pred = pred.to(torch.bfloat16).contiguous()
            if pruned:
                _ops().cfg_euler_nb(pred, nb, x, x_next, float(text_gs), float(image_gs), float(t_prev - t_curr), gvec)
            else:
                _ops().cfg_euler(pred, x, x_next, float(text_gs), float(image_gs), float(t_prev - t_curr), gvec)
            x, x_next = x_next, x
        return x

    def prepare_guidance(self, text: list, optional_models: dict, device, dtype, **kwargs):
        ret = {"guidance_img": kwargs.pop("guidance_img")}
        neg = kwargs.get("neg", None)
        if neg is None:
            neg = [""] * len(text)
        return text + neg + neg, ret


class DistilledDenoiser:
    """sampling.py:246-279.  `denoise(model, img=..., timesteps=[...], guidance=..., img_ids=..., txt=..., txt_ids=..., y_vec=...)`:
    no CFG triple -- the guidance value goes into the model's guidance embedding (guidance_embed=True, the flux-dev image model of
    the t2i2v pipeline) and the Euler update `img + (t_prev - t_curr) * pred` runs in img's dtype with the reference's torch ops,
    so the state matches the reference's bit for bit for the same model outputs.

    Not in the reference: `hip_graph=True` replays the model forward of steps 1.. from a hipGraph captured after step 0, as in
    I2VDenoiser (the latent and the timestep vector live in fixed buffers).  Same results bit for bit."""

    def denoise(self, model, **kwargs) -> Tensor:
        img = kwargs.pop("img")
        timesteps = kwargs.pop("timesteps")
        guidance = kwargs.pop("guidance")
        hip_graph = bool(kwargs.pop("hip_graph", False))
        kwargs.pop("step_cache_coefficients", None)
        kwargs.pop("attn_broadcast_range", None)
        if kwargs.pop("attn_broadcast", None) is not None:
            # (the keyword only, as for step_cache below: OSK_ATTN_BROADCAST is I2VDenoiser's default)
            raise ValueError("attn_broadcast is out of scope for DistilledDenoiser: its loop has no step schedule to broadcast over")
        if kwargs.pop("step_cache", None) is not None:
            # (the keyword only: OSK_STEP_CACHE is I2VDenoiser's default and leaves the image stage of a t2i2v run alone)
            raise ValueError("step_cache is out of scope for DistilledDenoiser: its loop has no head / blocks / tail split")
        guidance_vec = torch.full((img.shape[0],), guidance, device=img.device, dtype=img.dtype)
        if not hip_graph:
            for t_curr, t_prev in zip(timesteps[:-1], timesteps[1:]):
                t_vec = torch.full((img.shape[0],), t_curr, dtype=img.dtype, device=img.device)
                pred = model(img=img, **kwargs, timesteps=t_vec, guidance=guidance_vec)
                img = img + (t_prev - t_curr) * pred
            return img
        dev = img.device
        side = _SIDE_STREAMS.get(str(dev))
        if side is None:
            side = _SIDE_STREAMS[str(dev)] = torch.cuda.Stream(dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            x = img.clone()                                   # the fixed input buffer of the captured forward
            t_vec = torch.empty(img.shape[0], dtype=img.dtype, device=dev)
            graph, pred = None, None
            for i, (t_curr, t_prev) in enumerate(zip(timesteps[:-1], timesteps[1:])):
                t_vec.fill_(t_curr)
                if graph is not None:
                    graph.replay()
                else:
                    pred = model(img=x, **kwargs, timesteps=t_vec, guidance=guidance_vec)
                    if i == 0 and len(timesteps) > 2:
                        graph = torch.cuda.CUDAGraph()
                        with torch.cuda.graph(graph, stream=side):
                            pred_g = model(img=x, **kwargs, timesteps=t_vec, guidance=guidance_vec)
                x.copy_(x + (t_prev - t_curr) * pred)
                if graph is not None:
                    pred = pred_g
        torch.cuda.current_stream(dev).wait_stream(side)
        return x

    def prepare_guidance(self, text: list, optional_models: dict, device, dtype, **kwargs):
        return text, {}


SamplingMethodDict = {
    "i2v": I2VDenoiser(),
    "distill": DistilledDenoiser(),
}
