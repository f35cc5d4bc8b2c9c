"""Sequence parallelism of the denoise step over the GPUs of one node (one process per GPU, RCCL over xGMI).

What the reference does (mmdit_model_forward, /root/reference/opensora/models/mmdit/distributed.py:580-683):
every rank receives the full inputs, keeps a contiguous 1/P chunk of the joint [txt ; img] token axis
(:609-624, `L % P == 0` asserted at :604-608), runs every token-wise op on its chunk, exchanges K/V inside
attention (ring P2P of KV chunks + LSE merge, :223-313, or Ulysses all-to-all, :473-495) and all-gathers the
prediction at the end (:678-679).

MI355X design: the exchange is ONE all-gather of K and of V^T per block instead of P-1 ring
hops — xGMI is a full point-to-point mesh, every rank can pull from all 7 peers at once, and the local flash
kernel then runs once over the whole key axis (segment-addressed: key j lives in gathered segment j / (L/P)), so
there is no per-hop LSE merge and no P small launches.  Every exchange runs on a SECOND HIP stream owned by the transport
(`DistTransport`: an event recorded on the compute stream behind the producing kernels, the collective issued on the
communication stream behind that event, a completion event the attention launch waits on -- stream-level, the host never
blocks), so the Q projection (+ the MLP-up projection in single blocks) runs on the compute stream beside the exchange.
No reduce-scatter is needed for inference (it is the backward of the all-gather).
The transport is an object (`all_gather / all_to_all / all_reduce_max`, each returning a handle with `wait()`): production =
`DistTransport` over `torch.distributed` (`nccl` = RCCL over xGMI); tests/local_transport.py runs P ranks as threads of ONE
process on ONE GPU with device-copy "collectives" on per-rank communication streams (tests/test_gpu_overlap.py), which
exercises the same event protocol and the overlap itself where no multi-GPU node is available.

Chunked gather (kv_chunks = S > 1, opt-in; all-gather mode with bf16 attention): the one launch cannot start before the last byte
of K and V^T has arrived, and only the Q projection (+ MLP-up) hides that.  The reference hides its exchange under attention itself
(ring: compute on one key block while the next travels, merge by log-sum-exp, distributed.py:223-313).  The xGMI form keeps the full
mesh: the gather is cut into S gathers over key sub-ranges (rows [s L/(P S), (s + 1) L/(P S)) of every rank), all issued up front on
the communication stream; attention launch s waits for gather s only and returns (out, lse); osk_attention_merge_bf16 combines the S
partials in one HBM-bound pass.  The cost side (S launches + the merge) is measured in profiles/sp_chunked.md; the hidden-exchange
side needs a multi-GPU node, so the default stays S = 1.

Head-parallel exchange ("ulysses", the reference's other mode, distributed.py:473-495): when the head count divides
by P the block can instead all-to-all q, k, v from "my tokens, all heads" to "all tokens, my H/P heads", run the flash
kernel on whole sequences of H/P heads and all-to-all the result back.  Per rank and block it moves
4 (P-1)/P local tensors instead of 2 (P-1) — 4x less at P = 8, 2x less at P = 4, the same at P = 2 — and xGMI's
bandwidth per link is what bounds this small-hidden-size model at P > 2, so "auto" picks it for P >= 4.
The received chunks stay in their [source rank][batch][token] order: keys are addressed as P segments (the kernel's
segment layout), queries as P*B batches that share B key sets (osk_attention_fwd_bf16's kv_batches), and the output
lands directly in the layout the return all-to-all sends — no re-layout pass on the receive side.

Equal chunks keep every collective a plain `all_gather_into_tensor` / `all_to_all_single`; the final prediction is gathered as
[P, B, L/P, C] (rank 0 also projects its text rows, which are dropped after the gather) instead of the
reference's var-len gather (:39-112).

Token counts P does not divide (the reference asserts them away, :604-608): ranks 0 .. P-2 own Lc = ceil(L / P) rows, the last rank the
Ltail = L - (P - 1) Lc that remain (SeqPar.split).  Every buffer above keeps P slots of Lc rows -- zero-filled once, the last rank writes
only its Ltail rows -- so the collectives do not change; token-wise work runs on the true row count; attention sees P - 1 key segments of
Lc keys and one of Ltail, which the kernels take as two launches and an in-place merge (osk_attention_fwd_ragged_bf16, bf16 / pv8 / qk8);
the gathered prediction [P, B, Lc, C] is cut to L rows.  P | L never takes that path.  kv_chunks is ignored on a ragged split.

Frame-window attention (MMDiTModel.set_attention_window, opt-in; both modes; bf16 here, fp8 mode below): the window entry takes one key segment,
so K and V travel token-major through the same collectives, osk_kv_join_bf16 lays the gathered segments out as K [B, L, D] and
V^T [B, H, hd, round_up(L, 64)], and the rank runs osk_attention_fwd_window_bf16 on the table of its own rows -- once per source
rank in head-exchange mode.  A ragged split is the join's short last segment.  See "frame-window attention" below.
With anchor frames (set_attention_window(anchors=...)) the spec carries them and the call is osk_attention_fwd_window_anchor_bf16.
In fp8 mode (enable_fp8: pv8, and qk8 at head_dim 128) what the kernels consume as e4m3 travels as e4m3, token-major: with the scales
of the unwindowed fp8 exchange (all-gather mode: one reducing collective per block) osk_kv_quant_rows_fp8 writes the rank's rows into
its slot of a byte gather buffer -- V always, K under qk8; under pv8 K travels bf16 -- and osk_kv_join_fp8 lays the gathered segments
out as vt8 [B, H, vt8_rows(hd), round_up(L, 64)] and k8 [B, H, round_up(L, 64), 128] (pv8: the bf16 K), bit for bit what
osk_v_transpose_fp8 / osk_k_pack_fp8 write for the contiguous tensors; then osk_attention_fwd_window_fp8_bf16 (or the anchored entry)
in that mode.  Head-exchange mode sends bf16 as without a window and quantises what it received, its scales without a collective.
"""
from __future__ import annotations

import os

import torch
import torch.distributed as dist
from torch import Tensor

from . import mmdit

BF16 = torch.bfloat16


class _Done:
    def wait(self):
        return True


class _EventWork:
    """completion of an exchange issued on the communication stream: wait() makes the CURRENT stream wait for it"""

    def __init__(self, event, device):
        self.event, self.device = event, device

    def wait(self):
        torch.cuda.current_stream(self.device).wait_event(self.event)
        return True


class DistTransport:
    """Collectives of one process group (`nccl` = RCCL in production, `gloo` in the CPU tests).  For device tensors every call
    is issued on this transport's communication stream behind an event of the calling (compute) stream and returns a handle
    whose wait() orders the caller's stream behind the exchange: compute queued between the call and the wait() overlaps it.
    The buffers handed in are persistent (SeqPar._bufs), so no allocator stream bookkeeping is needed."""

    def __init__(self, group=None, overlap: bool = True):
        self.group = group if group is not None else dist.group.WORLD
        self.P = dist.get_world_size(self.group)
        self.rank = dist.get_rank(self.group)
        self.overlap = overlap
        self._comm = {}

    def comm_stream(self, device):
        st = self._comm.get(str(device))
        if st is None:
            st = self._comm[str(device)] = torch.cuda.Stream(device)
        return st

    def _run(self, t: Tensor, fn):
        if not (t.is_cuda and self.overlap):
            fn()
            return _Done()
        cur, comm = torch.cuda.current_stream(t.device), self.comm_stream(t.device)
        ready = torch.cuda.Event()
        ready.record(cur)                    # everything queued so far (the kernels that produced the send buffer)
        with torch.cuda.stream(comm):
            comm.wait_event(ready)
            fn()                             # a synchronous collective orders `comm` behind the backend's own stream
            done = torch.cuda.Event()
            done.record(comm)
        return _EventWork(done, t.device)

    def all_gather(self, out: Tensor, inp: Tensor):
        """out (flat, P chunks) <- every rank's inp (flat, one chunk; may alias out's own chunk)"""
        return self._run(out, lambda: dist.all_gather_into_tensor(out, inp, group=self.group))

    def all_to_all(self, out: Tensor, inp: Tensor):
        """chunk s of out <- chunk `rank` of rank s's inp"""
        return self._run(out, lambda: dist.all_to_all_single(out, inp, group=self.group))

    def all_reduce_max(self, t: Tensor):
        """max over the ranks, in place (a few floats: the e4m3 scales of V in fp8 mode).  Issued on the communication stream like
        every other exchange (round 5 ran it as a blocking collective on the compute stream): what the caller queues before wait()
        -- the K copy into the gather buffer -- overlaps its latency."""
        return self._run(t, lambda: dist.all_reduce(t, op=dist.ReduceOp.MAX, group=self.group))


class SeqPar:
    """Per-model sequence-parallel state: process group + the gathered K / V^T buffers (allocated once per
    geometry, reused by all 28/57 blocks: 2 * B * L * D * 2 bytes)."""

    def __init__(self, group=None, mode: str | None = None, transport=None, kv_chunks: int | None = None):
        self.tp = transport if transport is not None else DistTransport(group)
        self.P, self.rank = self.tp.P, self.tp.rank
        self._bufs = {}
        self._win_tables = {}  # host tables of frame-window attention, per (geometry, W, rows): window_table()
        self.geom = None     # (Lc, Ltail) of the split shard_range() last made
        self.exposed = None   # a list while bench.py measures exposed communication (see _timed_wait)
        self.mode = mode or os.environ.get("OSK_SP_MODE", "auto")   # "allgather" | "ulysses" | "auto"
        if self.mode not in ("allgather", "ulysses", "auto"):
            raise ValueError(f"unknown sequence-parallel mode {self.mode!r}")
        # all-gather mode, bf16 attention: cut the K / V^T gather into up to `kv_chunks` key slices and run the attention slice by
        # slice behind their arrival (gather_kv_start / attention below).  1 = one gather, one launch, no merge.
        self.kv_chunks = int(os.environ.get("OSK_SP_KV_CHUNKS", "1") if kv_chunks is None else kv_chunks)
        if not 1 <= self.kv_chunks <= self.MAX_KV_CHUNKS:
            raise ValueError(f"kv_chunks must be in 1 .. {self.MAX_KV_CHUNKS}, not {self.kv_chunks}")

    # ------------------------------------------------------------------ exposed-communication accounting (bench.py --gpus N)
    def _timed_wait(self, work, what: str):
        """wait() on an exchange; with `self.exposed` set to a list, bracket the wait with two events on the compute stream: the
        time between them is what the compute stream STALLED for this exchange -- its exposed part (0 when the exchange finished
        behind the kernels queued in front of the wait).  Events only; the host does not block."""
        rec = self.exposed
        if rec is None or not torch.cuda.is_available():
            work.wait()
            return
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        work.wait()
        e1.record()
        rec.append((what, e0, e1))

    def exposed_summary(self) -> dict:
        """ms the compute stream stalled per exchange kind since `exposed` was set (call after a synchronize)"""
        out: dict = {}
        for what, e0, e1 in self.exposed or []:
            out[what] = out.get(what, 0.0) + e0.elapsed_time(e1)
        return {k: round(v, 3) for k, v in out.items()}

    def head_parallel(self, H: int) -> bool:
        """exchange heads (all-to-all) instead of gathering K / V^T?"""
        if self.mode == "ulysses":
            assert H % self.P == 0, f"Expected {H} % {self.P} == 0"   # distributed.py:477-479
            return True
        return self.mode == "auto" and H % self.P == 0 and self.P >= 4

    # ------------------------------------------------------------------ sharding
    def shard_range(self, L: int, L_txt: int):
        """Token range [lo, hi) of the joint sequence owned by this rank, or None when sharding must be
        skipped because some rank would hold no image tokens (the reference then disables SP for the call,
        distributed.py:617-619)."""
        self.geom = None
        if self.P == 1:
            return None
        Lc, Ltail = self.split(L)
        if Ltail < 1 or Lc <= L_txt:  # a rank without rows, or rank 0 text-only (`0 in img_splits`)
            return None
        self.geom = (Lc, Ltail)
        return self.rank * Lc, min((self.rank + 1) * Lc, L)

    def split(self, L: int):
        """(Lc, Ltail): ranks 0 .. P-2 own Lc = ceil(L / P) rows of the joint sequence, the last rank the Ltail = L - (P - 1) Lc that
        remain (Ltail == Lc when P divides L: the reference's equal split, the only one it accepts, distributed.py:604-608).  The
        padding sits on the last rank alone: every exchange buffer holds P slots of Lc rows, so the collectives stay equal-sized."""
        Lc = -(-L // self.P)
        return Lc, L - (self.P - 1) * Lc

    def _geom(self, Lloc: int):
        """(slot rows Lc, rows of the last rank) for a call on Lloc local rows: the split shard_range() last made when Lloc is this
        rank's share of it, else the equal split of a direct call"""
        g = self.geom
        if g is not None and Lloc == (g[1] if self.rank == self.P - 1 else g[0]):
            return g
        return Lloc, Lloc

    # ------------------------------------------------------------------ K/V exchange
    # exchange-buffer sets kept (least recently used first out).  A forward uses one set; the sampler's cfg_prune loop alternates
    # at most three batch sizes = three sets, so none is evicted under it (tests/test_cfg_prune_host.py counts)
    MAX_GEOMETRIES = 4
    kv_qk8 = True        # gather_kv_start takes qk8 (mmdit._sp_qk8 asks before it passes the argument)
    MAX_KV_CHUNKS = 8    # parts osk_attention_merge_bf16 takes

    def kv_chunks_for(self, Lloc: int) -> int:
        """key slices S the gather of a rank with Lloc rows is cut into: the largest S <= kv_chunks that divides Lloc -- equal
        slices keep every collective a plain all_gather_into_tensor (a prime Lloc: 1)"""
        Lc, Ltail = self._geom(Lloc)
        if Ltail != Lc:        # a ragged split keeps the single gather (its attention is two launches + a merge already)
            return 1
        return max(s for s in range(1, max(1, min(self.kv_chunks, Lloc)) + 1) if Lloc % s == 0)

    def kv_chunks_applied(self, H: int, pv8: bool = False, Lloc: int = 0, Ltail: int = 0) -> int:
        """the S attention() runs with (reporting: MMDiTModel.attention_report): head-exchange mode needs the whole sequence of a
        head and the fp8 handles the reduced e4m3 scale before the first key is used -- both keep the single gather, and so does a
        ragged split (Ltail: the last rank's rows, where they differ from Lloc)"""
        if self.head_parallel(H) or pv8 or (Ltail and Ltail != Lloc):
            return 1
        return self.kv_chunks_for(Lloc) if Lloc else self.kv_chunks

    def _cached(self, key, make):
        """exchange buffers of one (kind, geometry, device, stream), least-recently-used eviction: an i2v run that alternates between
        a few shapes keeps all of them (round 5 cleared the WHOLE cache when a fourth geometry appeared and re-allocated
        2 B L D buffers mid-loop); the set in use -- the one a captured hipGraph replays into -- is always the newest entry."""
        b = self._bufs.pop(key, None)
        if b is None:
            while len(self._bufs) >= self.MAX_GEOMETRIES:
                self._bufs.pop(next(iter(self._bufs)))
            b = make()
        self._bufs[key] = b
        return b

    # Every exchange buffer holds P slots of Lloc = Lc rows.  Ltail (the last rank's rows; Lloc when P divides the sequence) is part
    # of the cache key: with Ltail < Lloc the buffers are zero-filled at allocation and the last rank writes only its Ltail rows, so
    # the pad rows stay zero for as long as the set lives -- which holds for ONE (Lc, Ltail) geometry only.
    def _buffers(self, B: int, Lloc: int, H: int, hd: int, device, Ltail: int | None = None):
        Ltail = Lloc if Ltail is None else Ltail

        def make():
            Lp = (Lloc + 63) // 64 * 64
            return ((torch.zeros if Ltail != Lloc else torch.empty)(self.P, B, Lloc, H * hd, dtype=BF16, device=device),
                    torch.zeros(self.P, B, H, hd, Lp, dtype=BF16, device=device))

        return self._cached((B, Lloc, Ltail, H, hd, str(device), mmdit._stream_key(device)), make)

    def _buffers8(self, B: int, Lloc: int, H: int, hd: int, device, Ltail: int | None = None):
        Ltail = Lloc if Ltail is None else Ltail

        def make():
            Lp = (Lloc + 63) // 64 * 64
            return ((torch.zeros if Ltail != Lloc else torch.empty)(self.P, B, Lloc, H * hd, dtype=BF16, device=device),
                    torch.zeros(self.P, B, H, mmdit.ops().vt8_rows(hd), Lp, dtype=torch.uint8, device=device))

        return self._cached(("pv8", B, Lloc, Ltail, H, hd, str(device), mmdit._stream_key(device)), make)

    def _buffers_qk8(self, B: int, Lloc: int, H: int, hd: int, device, Ltail: int | None = None):
        """qk8 (head_dim 128): K travels packed as e4m3 too -- [P, B, H, Lp, 128] bytes, no bf16 K buffer -- plus the [2, B, H]
        scale buffer (K's scales, then V's) that the one reducing collective of the block works on"""
        Ltail = Lloc if Ltail is None else Ltail

        def make():
            ops = mmdit.ops()
            Lp = (Lloc + 63) // 64 * 64
            return ((torch.zeros if Ltail != Lloc else torch.empty)(self.P, *ops.k8_shape(B, H, Lloc, hd), dtype=torch.uint8, device=device),
                    torch.zeros(self.P, B, H, ops.vt8_rows(hd), Lp, dtype=torch.uint8, device=device),
                    torch.empty(2, B, H, dtype=torch.float32, device=device))

        return self._cached(("qk8", B, Lloc, Ltail, H, hd, str(device), mmdit._stream_key(device)), make)

    @staticmethod
    def _own_layout(slot: Tensor, rows: int, key_axis: int = 3) -> Tensor:
        """a slot [B, H, R, Lp(Lc)] (V^T; key_axis 3) or [B, H, Lp(Lc), 128] (e4m3 K; key_axis 2) of the gathered buffers as the
        tensor the transposing / packing kernels write for `rows` keys: the same memory, round_up(rows, 64) key positions.  The slot
        itself unless the last rank's shorter chunk ends in an earlier 64-key tile (osk_attention_fwd_ragged_bf16 reads the last
        segment in this layout)."""
        Lp = (rows + 63) // 64 * 64
        if slot.shape[key_axis] == Lp:
            return slot
        shape = list(slot.shape)
        shape[key_axis] = Lp
        n = 1
        for d in shape:
            n *= d
        return slot.reshape(-1)[:n].view(shape)

    def _buffers_chunked(self, B: int, Lloc: int, S: int, H: int, hd: int, device):
        """kv_chunks: the gather buffers cut into S key slices of Lc = Lloc / S rows -- K [S, P, B, Lc, D], V^T
        [S, P, B, H, hd, round_up(Lc, 64)] (zero-filled: the key padding of a ragged slice) -- and the S partial results the slices'
        attention launches write: out [S, B, Lloc, D] bf16 and lse [S, B, H, Lloc] f32 (S more images of this rank's rows)"""
        def make():
            Lc = Lloc // S
            Lcp = (Lc + 63) // 64 * 64
            return (torch.empty(S, self.P, B, Lc, H * hd, dtype=BF16, device=device),
                    torch.zeros(S, self.P, B, H, hd, Lcp, dtype=BF16, device=device),
                    torch.empty(S, B, Lloc, H * hd, dtype=BF16, device=device),
                    torch.empty(S, B, H, Lloc, dtype=torch.float32, device=device))

        return self._cached(("chunks", S, B, Lloc, H, hd, str(device), mmdit._stream_key(device)), make)

    def local_vt(self, B: int, Lloc: int, H: int, hd: int, device):
        """this rank's slot [B, H, hd, round_up(L/P, 64)] of the gathered V^T buffer (all-gather mode, bf16), or None: the projection
        may write V straight into it as V^T (osk_gemm_group_bf16's V^T task, round 6) -- gather_kv_start(..., vt_ready=True) then
        skips the osk_v_transpose_bf16 pass.  None with kv_chunks too: the V^T task writes ONE contiguous slot, the slices are S."""
        if self.head_parallel(H) or self.kv_chunks_for(Lloc) > 1:
            return None
        Lc, Ltail = self._geom(Lloc)
        if Ltail != Lc:   # ragged split: the slot in the layout of THIS rank's rows (columns past them stay zero: written by nobody)
            return self._own_layout(self._buffers(B, Lc, H, hd, device, Ltail)[1][self.rank], Lloc)
        return self._buffers(B, Lloc, H, hd, device)[1][self.rank]

    def _ragged_kv_start(self, k: Tensor, v: Tensor, H: int, hd: int, pv8: bool, vt_ready: bool, qk8: bool, Lc: int, Ltail: int):
        """gather_kv_start (all-gather mode) on a ragged split: the same exchanges over slots of Lc rows.  This rank writes its
        Lloc <= Lc rows; the last rank's slot keeps the layout of a tensor of Ltail keys (_own_layout) in front of its zero padding.
        One gather whatever kv_chunks says.  The handle carries Ltail for attention()."""
        ops = mmdit.ops()
        B, Lloc, _ = k.shape
        r = self.rank
        if qk8:
            k8_all, vt8_all, s2 = self._buffers_qk8(B, Lc, H, hd, k.device, Ltail)
            ops.kv_scale_fp8(k, v, H, hd, out=s2)
            self._timed_wait(self.tp.all_reduce_max(s2), "kvmax")
            ops.k_pack_fp8(k, s2[0], self._own_layout(k8_all[r], Lloc, 2), H, hd)
            wk = self.tp.all_gather(k8_all.view(-1), k8_all[r].view(-1))
            ops.v_transpose_fp8(v, s2[1], self._own_layout(vt8_all[r], Lloc), H, hd)
            wv = self.tp.all_gather(vt8_all.view(-1), vt8_all[r].view(-1))
            return "ragged", "qk8", (Lc, Ltail), k8_all, vt8_all, s2[0], s2[1], wk, wv
        if pv8:
            sv = mmdit.v_scale_fp8(v, H, hd)
            wmax = self.tp.all_reduce_max(sv)
            k_all, vt8_all = self._buffers8(B, Lc, H, hd, k.device, Ltail)
            ops.copy_rows(k, k_all[r][:, :Lloc])
            wk = self.tp.all_gather(k_all.view(-1), k_all[r].view(-1))
            self._timed_wait(wmax, "vmax")
            ops.v_transpose_fp8(v, sv, self._own_layout(vt8_all[r], Lloc), H, hd)
            wv = self.tp.all_gather(vt8_all.view(-1), vt8_all[r].view(-1))
            return "ragged", "pv8", (Lc, Ltail), k_all, vt8_all, None, sv, wk, wv
        k_all, vt_all = self._buffers(B, Lc, H, hd, k.device, Ltail)
        ops.copy_rows(k, k_all[r][:, :Lloc])
        if not vt_ready:
            ops.v_transpose(v, self._own_layout(vt_all[r], Lloc), H, hd)
        wk = self.tp.all_gather(k_all.view(-1), k_all[r].view(-1))
        wv = self.tp.all_gather(vt_all.view(-1), vt_all[r].view(-1))
        return "ragged", "bf16", (Lc, Ltail), k_all, vt_all, None, None, wk, wv

    def _ragged_attention(self, pending, q: Tensor, out: Tensor, H: int, hd: int, score_bound: float):
        """P - 1 key segments of Lc keys and a last one of Ltail: osk_attention_fwd_ragged_bf16 -- one launch over the full
        segments, one over the last, one in-place merge; the divisible case never comes here"""
        _, kind, (Lc, Ltail), k_all, vt_all, k_scale, v_scale, wk, wv = pending
        self._timed_wait(wk, "k")
        self._timed_wait(wv, "v")
        ops = mmdit.ops()
        B, Lloc, _ = q.shape
        ops.attention_fwd_ragged(q, k_all[0], vt_all, out, H, hd, hd ** -0.5, n_seg=self.P, seg_len=Lc, last_seg_len=Ltail,
                                 k_seg_stride=k_all.stride(0), vt_seg_stride=vt_all.stride(0), q_prescaled=True,
                                 workspace=ops.attention_ragged_workspace(B, H, Lloc, hd, q.device),
                                 score_bound=score_bound if kind == "bf16" else 0.0, k_scale=k_scale, v_scale=v_scale)

    def gather_kv_start(self, ws, k: Tensor, v: Tensor, H: int, hd: int, pv8: bool = False, vt_ready: bool = False,
                        qk8: bool = False, window=None):
        """k, v: this rank's [B, L/P, D] views (K already normed + rotated with GLOBAL positions).  Starts the
        exchange of K and V and returns the handles; the caller keeps computing.
        pv8 (fp8 mode): V travels as e4m3 V^T (half the bytes); its per-(batch, head) scale must be the same on
        every rank -- the kernel accumulates P.V across all key segments -- so the local absmax is max-reduced first.
        qk8 (with pv8, head_dim 128 only; anything else behaves as without it): K travels as e4m3 as well, packed by osk_k_pack_fp8
        with scales that are the same on every rank, so the gathered bytes are the ones a single device would pack (padding rows
        aside).  K's and V's scales come from one osk_kv_scale_fp8 launch into one [2, B, H] buffer: still ONE reducing collective."""
        pv8 = pv8 and hd in (72, 128)
        qk8 = qk8 and pv8 and hd == 128
        if window is not None:     # frame-window attention (mmdit passes the argument only with the window on)
            return self._window_kv_start(k, v, H, hd, pv8, vt_ready, window, qk8)
        if self.head_parallel(H):
            return self._heads_kv_start(k, v, H, hd, pv8, qk8)
        B, Lloc, _ = k.shape
        Lc, Ltail = self._geom(Lloc)
        if Ltail != Lc:
            return self._ragged_kv_start(k, v, H, hd, pv8, vt_ready, qk8, Lc, Ltail)
        if qk8:
            ops = mmdit.ops()
            k8_all, vt8_all, s2 = self._buffers_qk8(B, Lloc, H, hd, k.device)
            ops.kv_scale_fp8(k, v, H, hd, out=s2)
            # (the co-residency rule of the pv8 branch below: the only REDUCING collective of the block; both packs need its result,
            #  so the compute stream runs nothing under it)
            self._timed_wait(self.tp.all_reduce_max(s2), "kvmax")
            ops.k_pack_fp8(k, s2[0], k8_all[self.rank], H, hd)
            wk = self.tp.all_gather(k8_all.view(-1), k8_all[self.rank].view(-1))
            ops.v_transpose_fp8(v, s2[1], vt8_all[self.rank], H, hd)
            wv = self.tp.all_gather(vt8_all.view(-1), vt8_all[self.rank].view(-1))
            return "qk8", k8_all, vt8_all, s2, wk, wv
        if pv8:
            sv = mmdit.v_scale_fp8(v, H, hd)
            # (co-residency rule of INTEGRATION.md section 4: the only REDUCING collective of this file; until its wait() below the
            #  compute stream runs the K copy only -- no hand-scheduled MFMA kernel overlaps RCCL's reduction kernel)
            wmax = self.tp.all_reduce_max(sv)                         # on the communication stream ...
            k_all, vt8_all = self._buffers8(B, Lloc, H, hd, k.device)
            mmdit.ops().copy_rows(k, k_all[self.rank])
            wk = self.tp.all_gather(k_all.view(-1), k_all[self.rank].view(-1))   # ... with the K copy and K's gather behind it
            self._timed_wait(wmax, "vmax")
            mmdit.ops().v_transpose_fp8(v, sv, vt8_all[self.rank], H, hd)
            wv = self.tp.all_gather(vt8_all.view(-1), vt8_all[self.rank].view(-1))
            return "pv8", k_all, vt8_all, sv, wk, wv
        S = self.kv_chunks_for(Lloc)
        if S > 1:
            # S gathers over key sub-ranges, all issued up front on the communication stream (the full mesh stays: no ring hops);
            # slice s = rows [s Lc, (s + 1) Lc) of EVERY rank.  The gather of slice s is issued before the copies of slice s + 1 are
            # queued, so it travels beside them -- and beside the Q projection -- and attention() starts on slice 0 while 1 .. S-1 travel
            assert not vt_ready, "local_vt() is None with kv_chunks: the projection writes V token-major"
            ops = mmdit.ops()
            k_all, vt_all, parts, lses = self._buffers_chunked(B, Lloc, S, H, hd, k.device)
            Lc = Lloc // S
            works = []
            for s in range(S):
                rows = slice(s * Lc, (s + 1) * Lc)
                ops.copy_rows(k[:, rows], k_all[s, self.rank])
                ops.v_transpose(v[:, rows], vt_all[s, self.rank], H, hd)
                wk = self.tp.all_gather(k_all[s].view(-1), k_all[s, self.rank].view(-1))
                wv = self.tp.all_gather(vt_all[s].view(-1), vt_all[s, self.rank].view(-1))
                works.append((wk, wv))
            return "chunks", k_all, vt_all, parts, lses, works
        k_all, vt_all = self._buffers(B, Lloc, H, hd, k.device)
        mmdit.ops().copy_rows(k, k_all[self.rank])
        if not vt_ready:                       # (vt_ready: the V projection already wrote local_vt())
            mmdit.ops().v_transpose(v, vt_all[self.rank], H, hd)
        wk = self.tp.all_gather(k_all.view(-1), k_all[self.rank].view(-1))
        wv = self.tp.all_gather(vt_all.view(-1), vt_all[self.rank].view(-1))
        return k_all, vt_all, wk, wv

    def attention(self, ws, pending, q: Tensor, out: Tensor, H: int, hd: int, score_bound: float = 0.0):
        """Local queries against the gathered keys: one launch, P key segments of L/P keys.  score_bound: the block's bound on
        |q . k| (mmdit._score_bound; it holds for every key of the joint sequence whichever rank projected it) -- the kernel's
        FAST body takes segmented / ragged key layouts since round 4, so sequence-parallel calls run it too."""
        if isinstance(pending[0], str) and pending[0] == "window":
            return self._window_attention(pending, q, out, H, hd, score_bound)
        if isinstance(pending[0], str) and pending[0] == "heads":
            return self._heads_attention(pending, q, out, H, hd, score_bound)
        if isinstance(pending[0], str) and pending[0] == "ragged":
            return self._ragged_attention(pending, q, out, H, hd, score_bound)
        B, Lloc, D = q.shape
        ops = mmdit.ops()
        if isinstance(pending[0], str) and pending[0] == "qk8":
            _, k8_all, vt8_all, s2, wk, wv = pending
            self._timed_wait(wk, "k")
            self._timed_wait(wv, "v")
            ops.attention_fwd_qk8(q, k8_all[0], s2[0], vt8_all, s2[1], out, H, hd, hd ** -0.5, seg_len=Lloc, n_seg=self.P,
                                  k_seg_stride=k8_all.stride(0), vt_seg_stride=vt8_all.stride(0), q_prescaled=True,
                                  workspace=ops.attention_workspace(q.device))
            return
        if isinstance(pending[0], str) and pending[0] == "chunks":
            # slice s: P key segments of Lc keys, its own wait -- the launch on slice s runs while slices s + 1 .. travel -- into
            # partial s with its log-sum-exp; ONE merge launch combines them (distributed.py:223-313 merges hop by hop)
            _, k_all, vt_all, parts, lses, works = pending
            Lc = k_all.shape[3]
            wsp = ops.attention_workspace(q.device)
            for s, (wk, wv) in enumerate(works):
                self._timed_wait(wk, "k")
                self._timed_wait(wv, "v")
                ops.attention_fwd(q, k_all[s, 0], vt_all[s], parts[s], H, hd, hd ** -0.5, lse=lses[s], n_seg=self.P, seg_len=Lc,
                                  k_seg_stride=k_all.stride(1), vt_seg_stride=vt_all.stride(1), q_prescaled=True,
                                  workspace=wsp, score_bound=score_bound)
            ops.attention_merge(parts, lses, out, H, hd)
            return
        if isinstance(pending[0], str):   # "pv8"
            _, k_all, vt8_all, sv, wk, wv = pending
            self._timed_wait(wk, "k")
            self._timed_wait(wv, "v")
            ops.attention_fwd_pv8(q, k_all[0], vt8_all, sv, out, H, hd, hd ** -0.5, n_seg=self.P, seg_len=Lloc,
                                  k_seg_stride=k_all.stride(0), vt_seg_stride=vt8_all.stride(0), q_prescaled=True,
                                  workspace=ops.attention_workspace(q.device))
            return
        k_all, vt_all, wk, wv = pending
        self._timed_wait(wk, "k")
        self._timed_wait(wv, "v")
        ops.attention_fwd(q, k_all[0], vt_all, out, H, hd, hd ** -0.5, n_seg=self.P, seg_len=Lloc,
                          k_seg_stride=k_all.stride(0), vt_seg_stride=vt_all.stride(0), q_prescaled=True,
                          workspace=ops.attention_workspace(q.device), score_bound=score_bound)

    # ------------------------------------------------------------------ head-parallel exchange (all-to-all)
    def _heads_buffers(self, B: int, Lloc: int, H: int, hd: int, device, Ltail: int | None = None):
        """send / receive chunks of Lloc = Lc rows.  Ragged split (Ltail < Lloc): zero-filled, and the last rank only ever writes its
        Ltail rows of a send chunk, so every received chunk of the last source rank ends in zero rows (finite scores and outputs)"""
        Ltail = Lloc if Ltail is None else Ltail

        def make():
            Hg, Lp = H // self.P, (Lloc + 63) // 64 * 64
            mk = lambda: (torch.zeros if Ltail != Lloc else torch.empty)(self.P, B, Lloc, Hg * hd, dtype=BF16, device=device)
            b = dict(ks=mk(), kr=mk(), vs=mk(), vr=mk(), qs=mk(), qr=mk(), os=mk(), orr=mk(), geom=(Lloc, Ltail),
                     vt=torch.zeros(self.P, B, Hg, hd, Lp, dtype=BF16, device=device))
            if hd in (72, 128):   # fp8 mode: e4m3 V^T of the received chunks
                b["vt8"] = torch.zeros(self.P, B, Hg, mmdit.ops().vt8_rows(hd), Lp, dtype=torch.uint8, device=device)
            return b

        return self._cached(("heads", B, Lloc, Ltail, H, hd, str(device), mmdit._stream_key(device)), make)

    def _to_head_chunks(self, dst: Tensor, x: Tensor):
        """[B, L/P, H*hd] (all heads of my tokens) -> dst [P, B, L/P, (H/P)*hd]: chunk j = head group j, for rank j.
        ONE osk_copy_rows_bf16 launch (chunk j of the source = columns j Dg ..): round 4 ran a torch permute-copy here, four per block."""
        B, Lloc, D = x.shape
        if dst.shape[2] != Lloc:      # the last rank of a ragged split: its rows lead the chunk, the rest stays zero
            dst = dst[:, :, :Lloc]
        mmdit.ops().copy_rows(x.view(B, Lloc, self.P, D // self.P).permute(2, 0, 1, 3), dst)

    def _from_head_chunks(self, out: Tensor, src: Tensor):
        """the way back: src [P, B, L/P, Dg] (head group j of my tokens, from rank j) -> out [B, L/P, P x Dg], head groups side by side"""
        B, Lloc, D = out.shape
        if src.shape[2] != Lloc:      # (the rows behind them were computed from zero queries: dropped here)
            src = src[:, :, :Lloc]
        mmdit.ops().copy_rows(src, out.view(B, Lloc, self.P, D // self.P).permute(2, 0, 1, 3))

    def _heads_kv_start(self, k: Tensor, v: Tensor, H: int, hd: int, pv8: bool = False, qk8: bool = False):
        """K and V travel in bf16 whatever the fp8 mode (packing K before the all-to-all would need per-segment K scales in the
        kernel); the handle's last element says what _heads_attention does with them: False, True (pv8) or "qk8" """
        B, Lloc, _ = k.shape
        Lc, Ltail = self._geom(Lloc)
        bufs = self._heads_buffers(B, Lc, H, hd, k.device, Ltail)
        if qk8:
            pv8 = "qk8"
            if "k8" not in bufs:    # e4m3 K of the received chunks: only a model that asked for qk8 pays for it
                bufs["k8"] = torch.empty(self.P, *mmdit.ops().k8_shape(B, H // self.P, Lc, hd), dtype=torch.uint8, device=k.device)
        self._to_head_chunks(bufs["ks"], k)
        wk = self.tp.all_to_all(bufs["kr"].view(-1), bufs["ks"].view(-1))
        self._to_head_chunks(bufs["vs"], v)
        wv = self.tp.all_to_all(bufs["vr"].view(-1), bufs["vs"].view(-1))
        return "heads", bufs, wk, wv, pv8

    def q_exchange_start(self, pending, q: Tensor, H: int, hd: int):
        """Head-parallel mode: start the all-to-all of the (normed, rotated, pre-scaled) queries and return the extended handle
        tuple -- whatever the caller queues before attention() overlaps it (single blocks: the MLP-up projection, the largest GEMM of
        the block; round 4 started this exchange inside attention() and waited on the spot).  All-gather mode: nothing to do."""
        if isinstance(pending[0], str) and pending[0] == "window" and pending[1] == "heads" and len(pending) == 7:
            bufs = pending[4]
            self._to_head_chunks(bufs["qs"], q)
            return (*pending, self.tp.all_to_all(bufs["qr"].view(-1), bufs["qs"].view(-1)))
        if not (isinstance(pending[0], str) and pending[0] == "heads") or len(pending) > 5:
            return pending
        bufs = pending[1]
        self._to_head_chunks(bufs["qs"], q)
        wq = self.tp.all_to_all(bufs["qr"].view(-1), bufs["qs"].view(-1))
        return (*pending, wq)

    def _heads_attention(self, pending, q: Tensor, out: Tensor, H: int, hd: int, score_bound: float = 0.0):
        pending = self.q_exchange_start(pending, q, H, hd)     # (a caller that did not start it earlier)
        _, bufs, wk, wv, pv8, wq = pending
        B, D = q.shape[0], q.shape[2]
        Lloc, Ltail = bufs["geom"]     # rows of a chunk (Lc), valid rows of the last source rank's
        if Ltail != Lloc:
            return self._heads_attention_ragged(pending, out, H, hd, score_bound)
        P, Hg = self.P, H // self.P
        self._timed_wait(wq, "q")
        self._timed_wait(wk, "k")
        self._timed_wait(wv, "v")
        # received chunk s = source rank s's tokens = key segment s; [P, B] is also the query "batch" axis
        ops = mmdit.ops()
        qr, kr, os_ = bufs["qr"].view(P * B, Lloc, Hg * hd), bufs["kr"], bufs["os"].view(P * B, Lloc, Hg * hd)
        if pv8 == "qk8":   # (the whole sequence of its heads is here: no collective for either scale vector)
            kr3, vr3 = kr.view(P * B, Lloc, Hg * hd), bufs["vr"].view(P * B, Lloc, Hg * hd)
            s2 = ops.kv_scale_fp8(kr3, vr3, Hg, hd).view(2, P, B, Hg).amax(1).contiguous()                      # [2, B, Hg]
            s2p = s2.repeat(1, P, 1)                                                                          # [2, P * B, Hg]
            k8, vt8 = bufs["k8"], bufs["vt8"]
            ops.k_pack_fp8(kr3, s2p[0], k8.view(P * B, Hg, k8.shape[-2], 128), Hg, hd)
            ops.v_transpose_fp8(vr3, s2p[1], vt8.view(P * B, Hg, vt8.shape[-2], vt8.shape[-1]), Hg, hd)
            ops.attention_fwd_qk8(qr, k8[0], s2[0], vt8, s2[1], os_, Hg, hd, hd ** -0.5, seg_len=Lloc, n_seg=P,
                                  k_seg_stride=k8.stride(0), vt_seg_stride=vt8.stride(0), q_prescaled=True, kv_batches=B,
                                  workspace=ops.attention_workspace(q.device))
        elif pv8:   # this rank holds the WHOLE sequence of its heads: the e4m3 scale needs no collective
            vr = bufs["vr"]
            sv = ops.v_scale_fp8(vr.view(P * B, Lloc, Hg * hd), Hg, hd).view(P, B, Hg).amax(0).contiguous()   # [B, Hg]
            vt8 = bufs["vt8"]
            ops.v_transpose_fp8(vr.view(P * B, Lloc, Hg * hd), sv.repeat(P, 1).contiguous(),
                                vt8.view(P * B, Hg, vt8.shape[-2], vt8.shape[-1]), Hg, hd)
            ops.attention_fwd_pv8(qr, kr[0], vt8, sv, os_, Hg, hd, hd ** -0.5, n_seg=P, seg_len=Lloc,
                                  k_seg_stride=kr.stride(0), vt_seg_stride=vt8.stride(0), q_prescaled=True, kv_batches=B,
                                  workspace=ops.attention_workspace(q.device))
        else:
            vt = bufs["vt"]
            ops.v_transpose(bufs["vr"].view(P * B, Lloc, Hg * hd), vt.view(P * B, Hg, hd, vt.shape[-1]), Hg, hd)
            ops.attention_fwd(qr, kr[0], vt, os_, Hg, hd, hd ** -0.5, n_seg=P, seg_len=Lloc, k_seg_stride=kr.stride(0),
                              vt_seg_stride=vt.stride(0), q_prescaled=True, kv_batches=B,
                              workspace=ops.attention_workspace(q.device), score_bound=score_bound)
        # chunk s of the output belongs to rank s's tokens: straight back, then head groups side by side
        self._timed_wait(self.tp.all_to_all(bufs["orr"].view(-1), bufs["os"].view(-1)), "o")
        self._from_head_chunks(out, bufs["orr"])

    def _heads_attention_ragged(self, pending, out: Tensor, H: int, hd: int, score_bound: float):
        """_heads_attention on a ragged split: P key segments of Lc rows of which the last holds Ltail, P * B query batches of Lc
        rows.  The last segment's V^T (and e4m3 K) is written by a call of its own over its Ltail keys -- the layout
        osk_attention_fwd_ragged_bf16 reads, and what keeps the zero pad rows out of the e4m3 validity row.  The pad queries of the
        last source rank's batches are zero rows: their outputs are finite and the return exchange's receiver drops them."""
        _, bufs, wk, wv, pv8, wq = pending
        Lc, Ltail = bufs["geom"]
        P, Hg = self.P, H // self.P
        B = bufs["qr"].shape[1]
        Dg = Hg * hd
        self._timed_wait(wq, "q")
        self._timed_wait(wk, "k")
        self._timed_wait(wv, "v")
        ops = mmdit.ops()
        qr, kr, vr, os_ = bufs["qr"].view(P * B, Lc, Dg), bufs["kr"], bufs["vr"], bufs["os"].view(P * B, Lc, Dg)
        full = lambda t: t[:P - 1].reshape((P - 1) * t.shape[1], *t.shape[2:])     # the P - 1 full segments as one batch axis (a view)
        k_last, v_last = kr[P - 1][:, :Ltail], vr[P - 1][:, :Ltail]
        k_op, k_scale, v_scale = kr, None, None
        if pv8:
            vt = bufs["vt8"]
            if pv8 == "qk8":
                s2 = ops.kv_scale_fp8(kr.view(P * B, Lc, Dg), vr.view(P * B, Lc, Dg), Hg, hd).view(2, P, B, Hg).amax(1).contiguous()   # [2, B, Hg]
                k_scale, v_scale = s2[0], s2[1]
                k_op = bufs["k8"]
                ops.k_pack_fp8(full(kr), k_scale.repeat(P - 1, 1).contiguous(), full(k_op), Hg, hd)
                ops.k_pack_fp8(k_last, k_scale, self._own_layout(k_op[P - 1], Ltail, 2), Hg, hd)
            else:
                v_scale = ops.v_scale_fp8(vr.view(P * B, Lc, Dg), Hg, hd).view(P, B, Hg).amax(0).contiguous()                         # [B, Hg]
            ops.v_transpose_fp8(full(vr), v_scale.repeat(P - 1, 1).contiguous(), full(vt), Hg, hd)
            ops.v_transpose_fp8(v_last, v_scale, self._own_layout(vt[P - 1], Ltail), Hg, hd)
        else:
            vt = bufs["vt"]
            ops.v_transpose(full(vr), full(vt), Hg, hd)
            ops.v_transpose(v_last, self._own_layout(vt[P - 1], Ltail), Hg, hd)
        ops.attention_fwd_ragged(qr, k_op[0], vt, os_, Hg, hd, hd ** -0.5, n_seg=P, seg_len=Lc, last_seg_len=Ltail,
                                 k_seg_stride=k_op.stride(0), vt_seg_stride=vt.stride(0), q_prescaled=True, kv_batches=B,
                                 workspace=ops.attention_ragged_workspace(P * B, Hg, Lc, hd, qr.device),
                                 score_bound=0.0 if pv8 else score_bound, k_scale=k_scale, v_scale=v_scale)
        self._timed_wait(self.tp.all_to_all(bufs["orr"].view(-1), bufs["os"].view(-1)), "o")
        self._from_head_chunks(out, bufs["orr"])

    # ------------------------------------------------------------------ frame-window attention (bf16 and fp8 mode, both exchange modes)
    # osk_attention_fwd_window_bf16 takes ONE key segment with the text prefix at keys [0, L_txt); the exchange buffers are
    # segment-major with segments that are no multiple of 64 keys.  K and V therefore travel token-major through the same collectives
    # (V instead of V^T: the same bytes), osk_kv_join_bf16 turns the gathered segments into K [B, L, D] and V^T [B, H, hd,
    # round_up(L, 64)] in one HBM-bound launch, and the window entry runs on the table of the query rows in hand (row0 = the owning
    # rank's first row): once in all-gather mode, once per source rank in head-exchange mode.  A ragged split is the join's short last
    # segment: the ragged two-launch entry is not used here.  No attention kernel and no generated loop differs for it.  fp8 mode:
    # _window_kv_start / _window_attention_fp8 -- the e4m3 operands travel as bytes, osk_kv_join_fp8 is the join.
    kv_window = True     # gather_kv_start takes window (mmdit asks before it passes the argument, like kv_qk8)

    def window_table(self, spec, row0: int, n_rows: int) -> Tensor:
        """host table of query rows [row0, row0 + n_rows) for spec = (L_txt, L_img, window_frames, frame_tokens) -- with anchor
        frames (L_txt, L_img, window_frames, frame_tokens, anchor_head, anchor_tail), the table then over the body keys between
        the always-attended ends: built once per (geometry, rows, W, anchors) and kept; the binding keeps its device copy by
        content (_C._window_on_device)"""
        key = (*spec, row0, n_rows)
        tabs = self._win_tables
        t = tabs.get(key)
        if t is None:
            while len(tabs) >= 64:
                tabs.pop(next(iter(tabs)))
            L_txt, L_img, W, N, *anchors = spec
            kw = dict(anchor_head=anchors[0], anchor_tail=anchors[1]) if anchors else {}
            t = tabs[key] = mmdit.attention_window_table(L_txt, L_img, N, W, row0=row0, n_rows=n_rows, **kw)
        return t

    def _window_buffers(self, B: int, Lc: int, Ltail: int, Hl: int, hd: int, Lq: int, device, gather: bool, anchored: bool = False):
        """per geometry, like the gather buffers: the joined K [B, L, Hl*hd] and V^T [B, Hl, hd, round_up(L, 64)] of the Hl heads this
        rank attends with, the window entry's workspace for calls of B batches of up to Lq rows, and (all-gather mode) the token-major
        gather buffers of K and V -- P slots of Lc rows; the join never reads the pad rows of a short last slot, so nothing is zeroed.
        anchored: the workspace of the anchored entry (two partial sets) instead -- a buffer set of its own per geometry"""
        def make():
            L = (self.P - 1) * Lc + Ltail
            ops = mmdit.ops()
            ws_bytes = (ops.attention_window_anchor_workspace_bytes if anchored else ops.attention_window_workspace_bytes)(B, Hl, Lq, hd)
            b = dict(kj=torch.empty(B, L, Hl * hd, dtype=BF16, device=device),
                     vtj=torch.empty(B, Hl, hd, (L + 63) // 64 * 64, dtype=BF16, device=device),
                     ws=torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=device))
            if gather:
                b["k"] = torch.empty(self.P, B, Lc, Hl * hd, dtype=BF16, device=device)
                b["v"] = torch.empty(self.P, B, Lc, Hl * hd, dtype=BF16, device=device)
            return b

        key = ("window", gather, B, Lc, Ltail, Hl, hd, Lq, str(device), mmdit._stream_key(device))
        return self._cached(key + (("anchored",) if anchored else ()), make)

    def _window_buffers8(self, B: int, Lc: int, Ltail: int, Hl: int, hd: int, Lq: int, device, gather: bool, fmode: str, anchored: bool = False):
        """_window_buffers in fp8 mode (fmode "pv8" | "qk8"): the joined e4m3 V^T [B, Hl, vt8_rows(hd), round_up(L, 64)] and K -- k8
        [B, Hl, round_up(L, 64), 128] under qk8, else the bf16 [B, L, Hl*hd] -- the window entry's workspace, and the token-major
        byte buffers the join reads: all-gather mode the gather buffers (V as e4m3; K as e4m3 under qk8, else bf16) and under qk8
        the [2, B, Hl] scale buffer of the block's one reducing collective; head-exchange mode the quantised received chunks.  The
        join writes every byte of its outputs and never reads the pad rows of a short last slot: nothing is zeroed."""
        def make():
            L = (self.P - 1) * Lc + Ltail
            ops = mmdit.ops()
            U8 = torch.uint8
            qk8 = fmode == "qk8"
            ws_bytes = (ops.attention_window_anchor_workspace_bytes if anchored else ops.attention_window_workspace_bytes)(B, Hl, Lq, hd)
            seg = lambda dt: torch.empty(self.P, B, Lc, Hl * hd, dtype=dt, device=device)
            b = dict(kj=torch.empty(ops.k8_shape(B, Hl, L, hd), dtype=U8, device=device) if qk8 else torch.empty(B, L, Hl * hd, dtype=BF16, device=device),
                     vtj=torch.empty(B, Hl, ops.vt8_rows(hd), (L + 63) // 64 * 64, dtype=U8, device=device),
                     ws=torch.empty(max(ws_bytes, 16), dtype=U8, device=device), v=seg(U8))
            if gather or qk8:        # (head-exchange mode under pv8: K is joined from the received bf16 chunks)
                b["k"] = seg(U8 if qk8 else BF16)
            if gather and qk8:
                b["s2"] = torch.empty(2, B, Hl, dtype=torch.float32, device=device)
            return b

        key = ("window8", fmode, gather, B, Lc, Ltail, Hl, hd, Lq, str(device), mmdit._stream_key(device))
        return self._cached(key + (("anchored",) if anchored else ()), make)

    kv_window_fp8 = True   # gather_kv_start takes window together with pv8 / qk8 (mmdit asks before it lets fp8 mode through)

    def _window_kv_start(self, k: Tensor, v: Tensor, H: int, hd: int, pv8: bool, vt_ready: bool, spec, qk8: bool = False):
        """fp8 mode (pv8; qk8 at head_dim 128): what the kernels consume as e4m3 travels as e4m3 -- token-major, quantised by
        osk_kv_quant_rows_fp8 straight into this rank's slot with the scales of the unwindowed fp8 exchange (one reducing collective
        per block) -- and osk_kv_join_fp8 lays the gathered segments out.  Head-exchange mode sends bf16 as ever (_heads_kv_start)
        and quantises what it received.  The handle's fourth element carries (Lc, Ltail, mode, k_scale, v_scale)."""
        ops = mmdit.ops()
        if pv8 and not (hasattr(ops, "kv_join_fp8") and hasattr(ops, "kv_quant_rows_fp8")):
            raise ValueError("frame-window attention under sequence parallelism: this kernel table has no fp8 join (kv_join_fp8 / "
                             "kv_quant_rows_fp8): enable_fp8(False) or set_attention_window(None)")
        fmode = "qk8" if qk8 else "pv8" if pv8 else "bf16"
        if self.kv_chunks > 1:
            raise ValueError(f"frame-window attention under sequence parallelism takes one gather: kv_chunks = {self.kv_chunks} is refused")
        assert not vt_ready, "local_vt() is not asked for with the window on: the projection writes V token-major"
        B, Lloc, _ = k.shape
        Lc, Ltail = self._geom(Lloc)
        if (self.P - 1) * Lc + Ltail != spec[0] + spec[1]:
            raise ValueError(f"frame-window attention: {self.P} ranks of {Lc} rows (last {Ltail}) are not the {spec[0]} + {spec[1]} rows of the window's geometry")
        if self.head_parallel(H):
            bufs = self._heads_buffers(B, Lc, H, hd, k.device, Ltail)
            self._to_head_chunks(bufs["ks"], k)
            wk = self.tp.all_to_all(bufs["kr"].view(-1), bufs["ks"].view(-1))
            self._to_head_chunks(bufs["vs"], v)
            wv = self.tp.all_to_all(bufs["vr"].view(-1), bufs["vs"].view(-1))
            return "window", "heads", spec, (Lc, Ltail, fmode, None, None), bufs, wk, wv
        r = self.rank
        if fmode != "bf16":
            bufs = self._window_buffers8(B, Lc, Ltail, H, hd, Lloc, k.device, True, fmode, anchored=len(spec) > 4)
            own = lambda t: t[r][:, :Lloc]
            if qk8:
                # (the co-residency rule of gather_kv_start's qk8 branch: the block's only REDUCING collective, both quantisations
                #  need its result, so the compute stream runs nothing under it)
                s2 = bufs["s2"]
                ops.kv_scale_fp8(k, v, H, hd, out=s2)
                self._timed_wait(self.tp.all_reduce_max(s2), "kvmax")
                k_scale, v_scale = s2[0], s2[1]
                ops.kv_quant_rows_fp8(k, k_scale, own(bufs["k"]), H, hd)
                wk = self.tp.all_gather(bufs["k"].view(-1), bufs["k"][r].view(-1))
            else:
                # (as gather_kv_start's pv8 branch: until the wait() the compute stream runs the K copy only)
                k_scale, v_scale = None, mmdit.v_scale_fp8(v, H, hd)
                wmax = self.tp.all_reduce_max(v_scale)
                ops.copy_rows(k, own(bufs["k"]))
                wk = self.tp.all_gather(bufs["k"].view(-1), bufs["k"][r].view(-1))
                self._timed_wait(wmax, "vmax")
            ops.kv_quant_rows_fp8(v, v_scale, own(bufs["v"]), H, hd)
            wv = self.tp.all_gather(bufs["v"].view(-1), bufs["v"][r].view(-1))
            return "window", "gather", spec, (Lc, Ltail, fmode, k_scale, v_scale), bufs, wk, wv
        bufs = self._window_buffers(B, Lc, Ltail, H, hd, Lloc, k.device, True, anchored=len(spec) > 4)
        ops.copy_rows(k, bufs["k"][r][:, :Lloc])
        wk = self.tp.all_gather(bufs["k"].view(-1), bufs["k"][r].view(-1))
        ops.copy_rows(v, bufs["v"][r][:, :Lloc])
        wv = self.tp.all_gather(bufs["v"].view(-1), bufs["v"][r].view(-1))
        return "window", "gather", spec, (Lc, Ltail, fmode, None, None), bufs, wk, wv

    def _window_attention(self, pending, q: Tensor, out: Tensor, H: int, hd: int, score_bound: float):
        """join, then the window entry: FAST body where the block's bound admits it, else the general one (the rule of
        mmdit._joint_attention's window path)"""
        pending = self.q_exchange_start(pending, q, H, hd)     # (head-exchange mode, a caller that did not start it earlier)
        _, kind, spec, (Lc, Ltail, fmode, k_scale, v_scale), bufs, wk, wv, *wq = pending
        P, L = self.P, (self.P - 1) * Lc + Ltail
        ops = mmdit.ops()
        if fmode != "bf16":
            return self._window_attention_fp8(pending, q, out, H, hd)
        bound = score_bound if 0.0 < score_bound <= mmdit.SCORE_BOUND_LIMIT else 0.0
        kw = dict(n_prefix=spec[0], q_prescaled=True, score_bound=bound)
        attend = ops.attention_fwd_window
        if len(spec) > 4:
            # anchor frames: the anchored entry on the joined K / V^T, its always-attended ends from the full sequence's geometry;
            # nothing differs in the exchange or the join
            n_prefix, n_suffix = mmdit.attention_window_bounds(spec[0], spec[1], spec[3], spec[4], spec[5])
            kw = dict(n_prefix=n_prefix, n_suffix=n_suffix, mode="bf16", q_prescaled=True, score_bound=bound)
            attend = ops.attention_fwd_window_anchor
        if kind == "gather":
            self._timed_wait(wk, "k")
            self._timed_wait(wv, "v")
            ops.kv_join(bufs["k"], bufs["v"], bufs["kj"], bufs["vtj"], H, hd, L)
            attend(q, bufs["kj"], bufs["vtj"], out, H, hd, hd ** -0.5, workspace=bufs["ws"],
                   windows=self.window_table(spec, self.rank * Lc, q.shape[1]), **kw)
            return
        B, Hg = q.shape[0], H // P
        jb = self._window_buffers(B, Lc, Ltail, Hg, hd, Lc, q.device, False, anchored=len(spec) > 4)
        self._timed_wait(wq[0], "q")
        self._timed_wait(wk, "k")
        self._timed_wait(wv, "v")
        ops.kv_join(bufs["kr"], bufs["vr"], jb["kj"], jb["vtj"], Hg, hd, L)
        # received query chunk p = source rank p's rows [p Lc, p Lc + rows): one call each with that rank's table, straight into the
        # slot the return all-to-all sends; the calls share the workspace (one stream, in order)
        for p_ in range(P):
            rows = Ltail if p_ == P - 1 else Lc
            attend(bufs["qr"][p_][:, :rows], jb["kj"], jb["vtj"], bufs["os"][p_][:, :rows], Hg, hd, hd ** -0.5,
                   workspace=jb["ws"], windows=self.window_table(spec, p_ * Lc, rows), **kw)
        self._timed_wait(self.tp.all_to_all(bufs["orr"].view(-1), bufs["os"].view(-1)), "o")
        self._from_head_chunks(out, bufs["orr"])

    def _window_attention_fp8(self, pending, q: Tensor, out: Tensor, H: int, hd: int):
        """_window_attention in fp8 mode: one osk_kv_join_fp8, then the fp8 window entry (the anchored entry with anchors set) in
        mode "pv8" | "qk8" with Lk = L and the scales every rank agrees on.  Head-exchange mode: the scales of the received chunks
        with no collective, as _heads_attention takes them (the zero pad rows of a ragged split move no maximum), the chunks
        quantised token-major, then the join and one call per source rank."""
        _, kind, spec, (Lc, Ltail, fmode, k_scale, v_scale), bufs, wk, wv, *wq = pending
        P, L = self.P, (self.P - 1) * Lc + Ltail
        ops = mmdit.ops()
        anchored = len(spec) > 4
        if anchored:
            n_prefix, n_suffix = mmdit.attention_window_bounds(spec[0], spec[1], spec[3], spec[4], spec[5])

        def attend(q_, jb, k_sc, v_sc, out_, Hl, table):
            if anchored:
                return ops.attention_fwd_window_anchor(q_, jb["kj"], jb["vtj"], out_, Hl, hd, hd ** -0.5, n_prefix=n_prefix, n_suffix=n_suffix,
                                                       windows=table, mode=fmode, k_scale=k_sc, v_scale=v_sc, q_prescaled=True,
                                                       workspace=jb["ws"], Lk=L)
            return ops.attention_fwd_window_fp8(q_, jb["kj"], k_sc, jb["vtj"], v_sc, out_, Hl, hd, hd ** -0.5, n_prefix=spec[0], windows=table,
                                                mode=fmode, q_prescaled=True, workspace=jb["ws"], Lk=L)

        if kind == "gather":
            self._timed_wait(wk, "k")
            self._timed_wait(wv, "v")
            ops.kv_join_fp8(bufs["k"], bufs["v"], bufs["kj"], bufs["vtj"], H, hd, L)
            attend(q, bufs, k_scale, v_scale, out, H, self.window_table(spec, self.rank * Lc, q.shape[1]))
            return
        B, Hg = q.shape[0], H // P
        Dg = Hg * hd
        jb = self._window_buffers8(B, Lc, Ltail, Hg, hd, Lc, q.device, False, fmode, anchored=anchored)
        self._timed_wait(wq[0], "q")
        self._timed_wait(wk, "k")
        self._timed_wait(wv, "v")
        kr3, vr3 = bufs["kr"].view(P * B, Lc, Dg), bufs["vr"].view(P * B, Lc, Dg)
        k_seg = bufs["kr"]
        if fmode == "qk8":
            s2 = ops.kv_scale_fp8(kr3, vr3, Hg, hd).view(2, P, B, Hg).amax(1).contiguous()                     # [2, B, Hg]
            k_scale, v_scale = s2[0], s2[1]
            ops.kv_quant_rows_fp8(kr3, k_scale.repeat(P, 1).contiguous(), jb["k"].view(P * B, Lc, Dg), Hg, hd)
            k_seg = jb["k"]
        else:
            v_scale = ops.v_scale_fp8(vr3, Hg, hd).view(P, B, Hg).amax(0).contiguous()                        # [B, Hg]
        ops.kv_quant_rows_fp8(vr3, v_scale.repeat(P, 1).contiguous(), jb["v"].view(P * B, Lc, Dg), Hg, hd)
        ops.kv_join_fp8(k_seg, jb["v"], jb["kj"], jb["vtj"], Hg, hd, L)
        for p_ in range(P):
            rows = Ltail if p_ == P - 1 else Lc
            attend(bufs["qr"][p_][:, :rows], jb, k_scale, v_scale, bufs["os"][p_][:, :rows], Hg, self.window_table(spec, p_ * Lc, rows))
        self._timed_wait(self.tp.all_to_all(bufs["orr"].view(-1), bufs["os"].view(-1)), "o")
        self._from_head_chunks(out, bufs["orr"])

    # ------------------------------------------------------------------ step cache
    step_cache = True    # gather_step_sums exists (mmdit._sp_step_cache_check asks before it lets the step cache run sharded, like kv_qk8)

    def gather_step_sums(self, pairs: Tensor) -> None:
        """pairs f32 [P, 2]: slot `rank` holds this rank's (sum |M_i - M_{i-1}|, sum |M_{i-1}|) in stream order; on return (stream
        order) every slot holds its rank's pair -- one all-gather of 8 bytes per rank, the step cache's only exchange of its own.
        Every rank then holds the same bits; osk_step_sums_combine_f32 adds them in rank order (MMDiTModel.step_head)."""
        self._timed_wait(self.tp.all_gather(pairs.view(-1), pairs[self.rank].view(-1)), "sums")

    # ------------------------------------------------------------------ output
    def gather_output(self, ws, project, C_out: int, L_txt: int) -> Tensor:
        """project(dst) writes this rank's [B, L/P, C_out] rows; returns the full image prediction
        [B, L_img, C_out] on every rank (gather_forward_split_backward_var_len, distributed.py:678-679)."""
        B, Lloc = ws.B, ws.L
        Lc, Ltail = self._geom(Lloc)
        # (ragged split: an exchange buffer like the others -- zero-filled, the last rank writes its Ltail rows only)
        full = (torch.zeros if Ltail != Lc else torch.empty)(self.P, B, Lc, C_out, dtype=BF16, device=ws.x.device)
        project(full[self.rank][:, :Lloc])
        self._timed_wait(self.tp.all_gather(full.view(-1), full[self.rank].view(-1)), "out")
        # (ragged split: the last slot's zero rows behind Ltail end behind row L, where the cut drops them)
        return full.permute(1, 0, 2, 3).reshape(B, self.P * Lc, C_out)[:, L_txt: (self.P - 1) * Lc + Ltail].contiguous()


def enable(model, group=None, mode: str | None = None, transport=None, kv_chunks: int | None = None) -> SeqPar:
    """Shard `model`'s denoise step over `group` (default: WORLD).  The counterpart of installing
    MMDiTPolicy / Distributed*Processor through booster.boost (distributed.py:686-760): weights stay replicated,
    MMDiTModel.forward keeps its signature and returns the full prediction on every rank.
    kv_chunks (default: OSK_SP_KV_CHUNKS, else 1): all-gather mode with bf16 attention cuts the K / V^T gather into that many key
    slices (the largest count <= kv_chunks that divides a rank's rows) and runs the attention slice by slice behind their arrival,
    merged by log-sum-exp; 1 = one gather and one launch.  Head-exchange mode and the fp8 attention ignore it."""
    sp = SeqPar(group, mode, transport, kv_chunks)
    model._sp = sp if sp.P > 1 else None
    return sp


def disable(model) -> None:
    model._sp = None
