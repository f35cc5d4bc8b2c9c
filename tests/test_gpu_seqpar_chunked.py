"""GPU (one GPU, P ranks as threads over tests/local_transport.py): seqpar.enable(..., kv_chunks=S) -- the K / V^T all-gather cut
into S key slices, one flash launch per slice behind its own gather, one osk_attention_merge_bf16 launch.

Tolerance, everywhere below: with e_1 = the error of the unchunked (S = 1) path and e_S = the error of the chunked path, on the
same inputs against the same reference (the f64 attention of tests/cpu_ops_attn_f64.py over the full key set for the op cases, the
single-device forward for the model cases), require  e_S <= max(1.5 e_1, 2^-8)  -- the project's parity rule.
The partials add S bf16 roundings under convex weights, so a ratio near 1 is expected; both values are printed."""
import copy

import pytest
import torch

from tests import cpu_ops_attn_f64 as F64
from tests.local_transport import LocalTransport, run_ranks
from tests.util import rel_l2, torch_inputs, torch_params

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
DEV = "cuda:0"


# ----------------------------------------------------------------------------------------------- op level
def _unit_rows(x, H, hd, norm):
    """rows of norm `norm` per head, so that |q . k| <= |q| |k| is known"""
    B, L, _ = x.shape
    xh = x.reshape(B, L, H, hd)
    return (xh / xh.norm(dim=-1, keepdim=True) * norm).reshape(B, L, H * hd)


_OP_REF: dict = {}


def _op_case(hd, P, Lloc):
    """operands of one rank-0 call and the f64 reference over the full key set: computed once per case, shared, never modified"""
    key = (hd, P, Lloc)
    if key not in _OP_REF:
        H, B = 2, 2
        g = torch.Generator().manual_seed(hd * 1000 + Lloc)
        q = _unit_rows(torch.randn(B, Lloc, H * hd, generator=g), H, hd, 4.0).to(BF)              # log2 units (q_prescaled)
        k = _unit_rows(torch.randn(P * B, Lloc, H * hd, generator=g), H, hd, 4.0).to(BF).reshape(P, B, Lloc, H * hd)
        v = torch.randn(P, B, Lloc, H * hd, generator=g).to(BF)
        ref = F64.reference(F64.heads(q.float(), H, hd), F64.mfma_k(k, H, hd, "bf16"), F64.mfma_v(v, H, hd, "bf16"), "bf16")
        exact = ref["out"].permute(0, 2, 1, 3).reshape(B, Lloc, H * hd)                              # f64 [B, Lloc, D]
        _OP_REF[key] = (H, B, q, k, v, exact)
    return _OP_REF[key]


@pytest.mark.parametrize("bounded", [False, True], ids=["general", "score_bound"])
@pytest.mark.parametrize("P,Lloc,S", [(2, 192, 3), (2, 200, 2)], ids=["Lc64", "Lc100_ragged"])
@pytest.mark.parametrize("hd", [72, 128])
def test_chunked_attention_of_a_rank_against_f64(hip_lib, hd, P, Lloc, S, bounded):
    """SeqPar.gather_kv_start + SeqPar.attention on every rank (rank r holds keys r Lloc ..; all ranks ask with the same queries),
    kv_chunks = 1 and kv_chunks = S, against the f64 attention over all P Lloc keys.  Lloc 192 / S 3: slices of one whole 64-key
    tile; Lloc 200 / S 2: slices of 100 keys -- a ragged second tile and a V^T padded to 128."""
    from open_sora_amd import seqpar

    H, B, q, k, v, exact = _op_case(hd, P, Lloc)
    # |q . k| <= 16 in log2 units by construction (+ the bf16 rounding of the rows); 0 = no promise, the general body
    bound = 16.5 if bounded else 0.0

    def run(chunks):
        def rank_fn(rank, world):
            sp = seqpar.SeqPar(mode="allgather", transport=LocalTransport(world, rank, DEV), kv_chunks=chunks)
            assert sp.kv_chunks_for(Lloc) == chunks
            qd, kd, vd = q.to(DEV), k[rank].to(DEV), v[rank].to(DEV)
            out = torch.empty(B, Lloc, H * hd, dtype=BF, device=DEV)
            for _ in range(2):                                              # twice: the buffers are reused block after block
                pending = sp.gather_kv_start(None, kd, vd, H, hd)
                assert (pending[0] == "chunks") == (chunks > 1)
                out.zero_()
                sp.attention(None, pending, qd, out, H, hd, bound)
            torch.cuda.current_stream().synchronize()
            return out.cpu()

        res = run_ranks(P, rank_fn, DEV)
        for o in res[1:]:
            assert torch.equal(o, res[0])                                   # same queries, same key set on every rank
        return res[0]

    o1, oS = run(1), run(S)
    e1, eS = rel_l2(o1.double(), exact), rel_l2(oS.double(), exact)
    print(f"hd {hd} P {P} Lloc {Lloc} S {S} bound {bound}: e_1 {e1:.3e} e_S {eS:.3e} ratio {eS / e1:.3f}")
    assert torch.isfinite(oS.float()).all()
    assert eS <= max(1.5 * e1, 2.0 ** -8), (eS, e1)


# ----------------------------------------------------------------------------------------------- model level
def _cfg():
    from oracle import configs

    return dict(configs.GOLDEN["hd72_eager_split"][0], depth=1, depth_single_blocks=1)


_MODEL: dict = {}


def _model_and_single(B):
    """the model, its inputs at L = 320 (T 4, 8 x 8 patches, 64 text tokens) and the single-device forward: once per batch size"""
    from open_sora_amd import mmdit

    if B not in _MODEL:
        cfg = _cfg()
        model = mmdit.Flux(device_map=DEV, torch_dtype=BF, **cfg)
        model.load_state_dict(torch_params(cfg, dtype=BF, device=DEV), strict=True)
        inp = torch_inputs(cfg, B, 4, 8, 8, 64, dtype=BF, device=DEV)
        with torch.inference_mode():
            single = model(**inp).float().cpu()                              # also builds the (shared, read-only) plan
        torch.cuda.synchronize()
        _MODEL[B] = (model, inp, single)
    return _MODEL[B]


@pytest.mark.parametrize("P,B", [(2, 2), (4, 1)], ids=["w2", "w4"])
def test_chunked_forward_against_the_single_device_forward(hip_lib, P, B):
    """the harness of tests/test_gpu_overlap.py (ranks as threads, own compute and communication streams, overlapped exchange) at
    L = 320, depth 1 + 1: 160 / 80 rows per rank, S = 2 -> slices of 80 / 40 keys"""
    from open_sora_amd import seqpar

    model, inp, single = _model_and_single(B)
    Lloc = 320 // P

    def run(chunks):
        def rank_fn(rank, world):
            m = copy.copy(model)
            m.forward = m.forward_ckpt
            object.__setattr__(m, "_osk_ws_cache", {})
            sp = seqpar.enable(m, mode="allgather", transport=LocalTransport(world, rank, DEV), kv_chunks=chunks)
            assert sp.kv_chunks_for(Lloc) == chunks and m.attention_report(P, Lloc)["kv_chunks"] == chunks
            with torch.inference_mode():
                outs = [m(**inp).float() for _ in range(2)]
            torch.cuda.current_stream().synchronize()
            return [o.cpu() for o in outs]

        res = run_ranks(P, rank_fn, DEV)
        for outs in res:
            assert torch.equal(outs[0], outs[1]), "sequence-parallel forward is not repeatable"
            assert torch.equal(outs[0], res[0][0]), "ranks disagree on the gathered prediction"
        return res[0][0]

    o1, oS = run(1), run(2)
    e1, eS = rel_l2(o1, single), rel_l2(oS, single)
    print(f"P {P} B {B} L 320 S 2: e_1 {e1:.3e} e_S {eS:.3e} ratio {eS / max(e1, 1e-30):.3f}")
    assert eS <= max(1.5 * e1, 2.0 ** -8), (eS, e1)


class _EchoTransport:
    """a rank whose peers echo it: every collective runs on the caller's stream with this rank's own chunk in every slot.  One
    thread, one stream, no events from other ranks -- what a stream capture needs (a capture cannot wait for an event recorded
    outside it, which the thread transport's cross-rank protocol does).  The forward is then attention over P copies of the rank's
    own keys: not the model's prediction, but the same launches, buffers and slice bookkeeping as a real rank's."""

    class _Done:
        def wait(self):
            return True

    def __init__(self, P, rank):
        self.P, self.rank = P, rank

    def all_gather(self, out, inp):
        o = out.view(self.P, -1)
        for s in range(self.P):
            if o[s].data_ptr() != inp.data_ptr():
                o[s].copy_(inp.view(-1))
        return self._Done()

    def all_reduce_max(self, t):
        return self._Done()


def test_chunked_forward_is_graph_capturable(hip_lib):
    """one rank's chunked forward (S = 2: two slice launches with lse + the merge per block) captured in a torch.cuda.graph and
    replayed == the eager result, bit for bit"""
    from open_sora_amd import seqpar

    model, inp, _ = _model_and_single(2)
    m = copy.copy(model)
    m.forward = m.forward_ckpt
    object.__setattr__(m, "_osk_ws_cache", {})
    sp = seqpar.enable(m, mode="allgather", transport=_EchoTransport(2, 0), kv_chunks=2)
    assert sp.kv_chunks_for(160) == 2
    with torch.inference_mode():
        eager = m(**inp).clone()
        torch.cuda.synchronize()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            m(**inp)                               # side-stream warm-up, as torch's capture recipe asks
        torch.cuda.current_stream().wait_stream(s)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            res = m(**inp)
        for _ in range(2):
            res.zero_()
            graph.replay()
            torch.cuda.synchronize()
            assert torch.isfinite(res.float()).all() and torch.equal(res, eager), "hipGraph replay differs from the eager forward"
