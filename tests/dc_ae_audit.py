"""TEST INFRASTRUCTURE ONLY -- a launch auditor for the Video DC-AE decoder (open_sora_amd.dc_ae, csrc/dc_ae.hip).

`Auditor(table)` is a proxy over a kernel table (open_sora_amd._C on the GPU, tests/cpu_ops_dc_ae on the CPU), installed with
mmdit.set_ops_for_testing.  It forwards the eight entry points a decode uses; after every call it synchronises, evaluates the
matching tests/cpu_ops_dc_ae `*_ref` formula in float64 on the device of the tensors the launch read, and judges the tensor the
launch wrote.  It keeps no tensor: one record (text and a few floats) per launch.

The bound is the one of tests/test_gpu_dc_ae.py, |out - y| <= 2^-8 |y| + 1e-4 max|y| (one bf16 rounding is 2^-9 relative; twice
that, plus 1e-4 of the largest output for the f32 accumulation); conv and depthwise launches report and assert the zero-padded
border and the interior separately.  dup_shuffle is a pure gather and must be bit-equal.

That bound was chosen for unit-normal inputs.  The inputs of launch 40 of a real chain are not, and f32 accumulation alone may
exceed 1e-4 max|y| under heavy cancellation.  So every launch also gets a CONTROL that never involves the kernel: the same `*_ref`
in float32, rounded once to bf16, judged by the same bound.  Where the control is inside the bound the kernel must be too.  Where
the control itself is outside, the kernel is judged by max-abs(kernel) <= 2 max-abs(control) in that region (one more bf16 rounding
on top of a different summation order), the launch is named "fallback" in the report, and at most FALLBACK_SHARE of the launches
of a decode may take that route -- a condition on the test's weights and latent, checked by `check()`.
"""
from __future__ import annotations

import time
from collections import Counter

import torch

from tests import cpu_ops_dc_ae as E

BF = torch.bfloat16
FALLBACK_SHARE = 0.10
ENTRY_POINTS = ("conv3d_zp", "dup_shuffle", "dwconv3d", "gconv32", "relu_linear_attn", "rmsnorm_affine", "gemm", "blend")
SLAB_ELEMS = 1 << 27      # f64 elements of one operand slab of the conv reference (1 GiB)


# ------------------------------------------------------------------------------------------------------------------ the bound
def measure(out, y, border=None) -> dict:
    """out against the f64 value y under |out - y| <= 2^-8 |y| + 1e-4 max|y|.  -> finite, ymax, regions {name: (max-abs, ok)}
    ("all", or "border" / "interior" when a border mask is given), worst (index of the largest excess over the bound, on_border)"""
    o = out.double()
    err = (o - y).abs()
    ymax = float(y.abs().max())
    excess = err - (2.0 ** -8 * y.abs() + 1e-4 * ymax)
    del o
    regions = {}
    if border is None:
        regions["all"] = (float(err.max()), bool((excess <= 0).all()))
    else:
        border = border.expand_as(err)
        inner = ~border
        regions["border"] = (float(err[border].max()), bool((excess[border] <= 0).all()))
        if bool(inner.any()):
            regions["interior"] = (float(err[inner].max()), bool((excess[inner] <= 0).all()))
        else:
            regions["interior"] = (0.0, True)
    flat = int(torch.argmax(excess.reshape(-1)))            # NaN sorts as the maximum
    idx = tuple(int(i) for i in torch.unravel_index(torch.tensor(flat), excess.shape))
    on_border = None if border is None else bool(border[idx])
    return dict(finite=bool(torch.isfinite(out.float()).all()), ymax=ymax, regions=regions, worst=(idx, on_border))


def _judge(name, out, y, border=None):
    """|out - y| <= 2^-8 |y| + 1e-4 max|y| everywhere; border and interior reported and asserted separately"""
    m = measure(out, y, border)
    assert m["finite"], name
    if border is None:
        e, ok = m["regions"]["all"]
        print(f"{name}: max-abs {e:.3e} (max |y| {m['ymax']:.3e})")
        assert ok, f"{name}: off by up to {e:.3e}"
        return
    (e_b, ok_b), (e_i, ok_i) = m["regions"]["border"], m["regions"]["interior"]
    print(f"{name}: max-abs border {e_b:.3e} interior {e_i:.3e} (max |y| {m['ymax']:.3e})")
    assert ok_b, f"{name}: border voxels off by up to {e_b:.3e}"
    assert ok_i, f"{name}: interior off by up to {e_i:.3e}"


def conv_border(To, Ho, Wo, device):
    """[1, To, Ho, Wo, 1] mask of the output voxels of a k = 3 conv near a zero-padded face: the first and last frame, two rows
    and two columns (an upsampled conv's outermost SOURCE voxel is two output voxels wide)"""
    b = torch.zeros(To, Ho, Wo, dtype=torch.bool, device=device)
    b[:1], b[-1:] = True, True
    b[:, :2], b[:, -2:], b[:, :, :2], b[:, :, -2:] = True, True, True, True
    return b[None, :, :, :, None]


def dw_border(T, H, W, k, device):
    b = torch.zeros(T, H, W, dtype=torch.bool, device=device)
    p = k // 2
    b[:p], b[-p:], b[:, :p], b[:, -p:], b[:, :, :p], b[:, :, -p:] = (True,) * 6
    return b[None, :, :, :, None]


# --------------------------------------------------------------------------------------------------------------- references
def conv3d_zp_ref_slabs(x, w, bias, ksize, up_t, up_hw, silu, res, dtype, slab_elems=SLAB_ELEMS):
    """tests/cpu_ops_dc_ae.conv3d_zp_ref, evaluated over slabs of output frames with a halo of ksize // 2 frames so that no
    operand of the largest launch (128 -> 128 at 32 x 256 x 256) is held in `dtype` whole.  The halo's own outputs are dropped; at
    the two ends of the volume the formula's zero padding stands."""
    B, T, H, W, Cin = x.shape
    Cout = w.shape[0]
    To, Ho, Wo = T << int(up_t), H << int(up_hw), W << int(up_hw)
    step = max(1, slab_elems // (B * Ho * Wo * max(Cin, Cout)))
    if step >= To:
        return E.conv3d_zp_ref(x, w, bias, ksize, up_t, up_hw, silu, res, dtype=dtype)
    xu = x.repeat_interleave(2, 1) if up_t else x
    if up_hw:
        xu = xu.repeat_interleave(2, 2).repeat_interleave(2, 3)
    p = ksize // 2
    y = torch.empty(B, To, Ho, Wo, Cout, dtype=dtype, device=x.device)
    for t0 in range(0, To, step):
        t1 = min(To, t0 + step)
        a, b = max(0, t0 - p), min(To, t1 + p)
        ys = E.conv3d_zp_ref(xu[:, a:b], w, bias, ksize, False, False, silu, None if res is None else res[:, a:b], dtype=dtype)
        y[:, t0:t1] = ys[:, t0 - a: t1 - a]
        del ys
    return y


def gemm_ref(a, w, bias, dtype):
    """x @ w[:, :K].T + b"""
    y = a.to(dtype) @ w[:, : a.shape[-1]].to(dtype).T
    return y if bias is None else y + bias.to(dtype)


def blend_ref(a, b0, extent, dim, dtype):
    """b[.., y, ..] = a[.., -e + y, ..] (1 - y / e) + b[.., y, ..] (y / e) for y < e = min(extent, both lengths); the rest of b
    untouched (the formula of tests/test_gpu_vae.py::test_blend_kernel_vs_reference_formula)"""
    dim = dim % b0.ndim
    e = min(a.shape[dim], b0.shape[dim], extent)
    ref = b0.to(dtype)
    for yy in range(e):
        ia, ib = [slice(None)] * b0.ndim, [slice(None)] * b0.ndim
        ia[dim], ib[dim] = a.shape[dim] - e + yy, yy
        ref[tuple(ib)] = a[tuple(ia)].to(dtype) * (1 - yy / e) + b0[tuple(ib)].to(dtype) * (yy / e)
    return ref, e


def expected_census(cfg: dict) -> Counter:
    """launches per entry point of ONE untiled decode, from the architecture (a tests/dc_ae_restatement.py configuration) alone.
    "conv3d_zp/k3" and "conv3d_zp/k1" are counted apart; a 1x1x1 ConvLayer is a gemm where no SiLU follows and Cin % 64 == 0."""
    W, D = cfg["width_list"], cfg["depth_list"]
    n = len(W)
    c = Counter()

    def pointwise(cin, silu):
        c["conv3d_zp/k1" if (silu or cin % 64) else "gemm"] += 1

    c["conv3d_zp/k3"] += 1                                   # project_in
    c["dup_shuffle"] += 1
    for sid in range(n):
        if sid < n - 1 and D[sid] > 0:                       # upsample block: conv with the shortcut as its residual
            c["conv3d_zp/k3"] += 1
            c["dup_shuffle"] += 1
        for _ in range(D[sid]):
            if cfg["block_type"][sid] == "ResBlock":
                c["conv3d_zp/k3"] += 2
                c["rmsnorm_affine"] += 1
            else:
                pointwise(W[sid], False)                     # qkv
                c["dwconv3d"] += 1                           # aggreg 5x5x5
                c["gconv32"] += 1
                c["relu_linear_attn"] += 2                   # two scales
                pointwise(2 * W[sid], False)                 # proj
                c["rmsnorm_affine"] += 1
                pointwise(W[sid], True)                      # inverted_conv + SiLU
                c["dwconv3d"] += 1                           # depth_conv + GLU
                pointwise(4 * W[sid], False)                 # point_conv
                c["rmsnorm_affine"] += 1
    c["rmsnorm_affine"] += 1                                 # project_out
    c["conv3d_zp/k3"] += 1
    return c


# ------------------------------------------------------------------------------------------------------------------ the proxy
class Auditor:
    def __init__(self, table, verbose: bool = False):
        self._table = table
        self.verbose = verbose
        self.records: list = []     # one dict per launch: n, entry, key, desc, errs, ymax, route, ok, why
        self.t0 = time.time()

    def __getattr__(self, name):
        v = getattr(self._table, name)
        if callable(v) and not isinstance(v, type):
            raise AttributeError(f"dc_ae_audit: entry point {name!r} is not audited (a decode may use only {ENTRY_POINTS})")
        return v

    # ---- bookkeeping
    @staticmethod
    def _sync(t):
        if t.is_cuda:
            torch.cuda.synchronize(t.device)

    def _record(self, entry, key, desc, out, y, ctrl, border=None, exact=None):
        """judge `out` (what the launch wrote) and `ctrl` (f32 formula rounded once to bf16) against y (f64)"""
        rec = dict(n=len(self.records), entry=entry, key=key, desc=desc, route="control", ok=True, why="", errs="", ymax=0.0)
        if exact is not None:                                 # pure gather: bit-equal
            rec["ok"] = bool(torch.equal(out, exact))
            rec["route"] = "exact"
            rec["errs"] = "bit-equal" if rec["ok"] else "NOT bit-equal"
            if not rec["ok"]:
                bad = (out != exact).nonzero()[0]
                rec["why"] = f"first differing element {tuple(int(i) for i in bad)}"
        else:
            k, c = measure(out, y, border), measure(ctrl, y, border)
            rec["ymax"] = k["ymax"]
            parts = []
            for name, (e_k, ok_k) in k["regions"].items():
                e_c, ok_c = c["regions"][name]
                if ok_c:
                    good = ok_k
                    rule = "bound"
                else:
                    good = e_k <= 2.0 * e_c
                    rule = "2 x control"
                    rec["route"] = "fallback"
                parts.append(f"{name} {e_k:.3e} (control {e_c:.3e})")
                if not good or not k["finite"]:
                    rec["ok"] = False
                    idx, on_border = k["worst"]
                    where = "" if on_border is None else (", on a border" if on_border else ", in the interior")
                    rec["why"] += (f"{name}: max-abs {e_k:.3e} fails the {rule} rule (control {e_c:.3e}); worst element "
                                   f"{_coords(idx)}{where}; ")
            rec["errs"] = " ".join(parts)
        self.records.append(rec)
        if self.verbose:
            print(self._line(rec), flush=True)

    @staticmethod
    def _line(r):
        return (f"{r['n']:4d} {r['entry']:<17s} {r['desc']:<78s} max-abs {r['errs']} max|y| {r['ymax']:.3e} {r['route']}"
                + ("" if r["ok"] else "  FAIL: " + r["why"]))

    # ---- the entry points
    def conv3d_zp(self, x, w, bias, out, ksize, up_t=False, up_hw=False, silu=False, res=None):
        r = self._table.conv3d_zp(x, w, bias, out, ksize, up_t, up_hw, silu, res)
        self._sync(out)
        y = conv3d_zp_ref_slabs(x, w, bias, ksize, up_t, up_hw, silu, res, torch.float64)
        ctrl = conv3d_zp_ref_slabs(x, w, bias, ksize, up_t, up_hw, silu, res, torch.float32).to(BF)
        flags = "".join(f for f, on in (("T", up_t), ("S", up_hw), ("b", bias is not None), ("s", silu), ("r", res is not None)) if on)
        desc = f"x {tuple(x.shape)} -> {tuple(out.shape)} k{ksize} [{flags}]"
        self._record("conv3d_zp", f"conv3d_zp/k{ksize}", desc, out, y, ctrl,
                     conv_border(*out.shape[1:4], out.device) if ksize == 3 else None)
        return r

    def dup_shuffle(self, x, out, ft, fhw):
        r = self._table.dup_shuffle(x, out, ft, fhw)
        self._sync(out)
        desc = f"x {tuple(x.shape)} -> {tuple(out.shape)} ft{ft} fhw{fhw}"
        self._record("dup_shuffle", "dup_shuffle", desc, out, None, None, exact=E.dup_shuffle_ref(x, out.shape[-1], ft, fhw))
        return r

    def dwconv3d(self, x, w, bias, out, ksize, glu=False):
        r = self._table.dwconv3d(x, w, bias, out, ksize, glu)
        self._sync(out)
        y = E.dwconv3d_ref(x, w, bias, ksize, glu, dtype=torch.float64)
        ctrl = E.dwconv3d_ref(x, w, bias, ksize, glu, dtype=torch.float32).to(BF)
        desc = f"x {tuple(x.shape)} -> {tuple(out.shape)} k{ksize} [{'b' if bias is not None else ''}{'g' if glu else ''}]"
        self._record("dwconv3d", "dwconv3d", desc, out, y, ctrl, dw_border(*out.shape[1:4], ksize, out.device))
        return r

    def gconv32(self, x, w, out):
        r = self._table.gconv32(x, w, out)
        self._sync(out)
        y = E.gconv32_ref(x, w, dtype=torch.float64)
        ctrl = E.gconv32_ref(x, w, dtype=torch.float32).to(BF)
        self._record("gconv32", "gconv32", f"x {tuple(x.shape)}", out, y, ctrl)
        return r

    def relu_linear_attn(self, qkv, out, eps=1e-15, workspace=None):
        r = self._table.relu_linear_attn(qkv, out, eps, workspace)
        self._sync(out)
        cols = qkv.shape[2] // 3
        y = E.relu_linear_attn_ref(qkv, eps, dtype=torch.float64)
        ctrl = E.relu_linear_attn_ref(qkv, eps, dtype=torch.float32).to(BF)
        self._record("relu_linear_attn", "relu_linear_attn", f"qkv {tuple(qkv.shape)} -> {cols} of {out.stride(1)} columns",
                     out[:, :, :cols], y, ctrl)
        return r

    def rmsnorm_affine(self, x, weight, bias, out, eps=1e-5, res=None, relu=False):
        r = self._table.rmsnorm_affine(x, weight, bias, out, eps, res, relu)
        self._sync(out)
        y = E.rmsnorm_affine_ref(x, weight, bias, eps, res, relu, dtype=torch.float64)
        ctrl = E.rmsnorm_affine_ref(x, weight, bias, eps, res, relu, dtype=torch.float32).to(BF)
        desc = f"x {tuple(x.shape)} [{'R' if relu else ''}{'r' if res is not None else ''}]"
        self._record("rmsnorm_affine", "rmsnorm_affine", desc, out, y, ctrl)
        return r

    def gemm(self, a, w, bias, out):
        """as dc_ae._pointwise calls it: no residual, gate or GELU"""
        r = self._table.gemm(a, w, bias, out)
        self._sync(out)
        y = gemm_ref(a, w, bias, torch.float64)
        ctrl = gemm_ref(a, w, bias, torch.float32).to(BF)
        desc = f"a {tuple(a.shape)} w {tuple(w.shape)} [{'b' if bias is not None else ''}]"
        self._record("gemm", "gemm", desc, out, y, ctrl)
        return r

    def blend(self, a, b, extent, dim):
        b0 = b.clone()
        r = self._table.blend(a, b, extent, dim)
        self._sync(b)
        y, e = blend_ref(a, b0, extent, dim, torch.float64)
        ctrl = blend_ref(a, b0, extent, dim, torch.float32)[0].to(BF)
        self._record("blend", "blend", f"a {tuple(a.shape)} b {tuple(b.shape)} extent {extent} dim {dim}", b, y, ctrl)
        rest = [slice(None)] * b.ndim
        rest[dim % b.ndim] = slice(e, None)
        if not torch.equal(b[tuple(rest)], b0[tuple(rest)]):
            self.records[-1]["ok"] = False
            self.records[-1]["why"] += "wrote outside the seam; "
        return r

    # ---- results
    def census(self) -> Counter:
        return Counter(r["key"] for r in self.records)

    def failures(self) -> list:
        return [r for r in self.records if not r["ok"]]

    def fallback_share(self) -> float:
        return sum(r["route"] == "fallback" for r in self.records) / max(1, len(self.records))

    def report(self) -> str:
        """one line per launch, then the summary"""
        nf = sum(r["route"] == "fallback" for r in self.records)
        tail = (f"{len(self.records)} launches, {len(self.failures())} failed, {nf} judged by the 2 x control fallback "
                f"({100.0 * self.fallback_share():.1f} %, at most {100.0 * FALLBACK_SHARE:.0f} % allowed); audited wall time "
                f"{time.time() - self.t0:.1f} s (f64-bound, recorded only)")
        return "\n".join([self._line(r) for r in self.records] + [tail])

    def check(self, what: str = "decode"):
        """every failure of the run in one AssertionError, the first one named first; then the fallback condition"""
        bad = self.failures()
        if bad:
            lines = [f"{what}: {len(bad)} of {len(self.records)} launches failed; first: launch {bad[0]['n']} ({bad[0]['entry']})"]
            raise AssertionError("\n".join(lines + [self._line(r) for r in bad]))
        share = self.fallback_share()
        named = [f"{r['n']} {r['entry']}" for r in self.records if r["route"] == "fallback"]
        assert share <= FALLBACK_SHARE, (f"{what}: the f32 control itself misses the bound at {100 * share:.1f} % of the launches "
                                         f"({named}): choose another weight seed / latent, the bound does not move")


def _coords(idx) -> str:
    names = ("b", "t", "h", "w", "c") if len(idx) == 5 else tuple(f"i{j}" for j in range(len(idx)))
    return "(" + ", ".join(f"{n}={v}" for n, v in zip(names, idx)) + ")"
