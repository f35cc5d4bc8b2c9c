"""TEST INFRASTRUCTURE ONLY: the f64 restatement of osk_lora_merge_bf16 (include/osk.h) and the per-element criterion its tests
use.  Nothing here is measured from the kernel: the bound follows from the number formats.

  exact[n, k] = w[n, k] + sum_i scale_i sum_j B_i[n, j] A_i[j, k]                     (f64; the bf16 inputs are exact in it)
  mag[n, k]   = |w[n, k]| + sum_i |scale_i| sum_j |B_i[n, j]| |A_i[j, k]|

The kernel forms every bf16 x bf16 product exactly, sums in f32 and rounds ONCE to bf16.  Its f32 sum takes at most
sum_i r_i additions inside the MFMAs, one fma per adapter for the scale and one addition of W: sum r + n_adapters + 1 roundings
(one more for f32(scale_i) itself), each at most 2^-24 of a partial sum that mag bounds.  A factor 2 covers an MFMA accumulation
order and rounding mode that is not specified.  Then one rounding to bf16: half a bf16 ulp of the value.
  |out - exact| <= half_ulp_bf16(exact) + 2 (sum r + n_adapters + 2) 2^-24 mag
"""
import torch

BF = torch.bfloat16


def lora_merge_f64(w: torch.Tensor, adapters):
    """(exact, mag) as above; w bf16 / f32 [N, K], adapters = (A [r, K], B [N, r], scale) triples"""
    exact, mag = w.double().cpu(), w.double().abs().cpu()
    for a, b, s in adapters:
        a, b = a.double().cpu(), b.double().cpu()
        s = float(torch.tensor(s, dtype=torch.float32))        # the ABI carries the scale as f32
        exact = exact + s * (b @ a)
        mag = mag + abs(s) * (b.abs() @ a.abs())
    return exact, mag


def half_ulp_bf16(x: torch.Tensor) -> torch.Tensor:
    """half a bf16 ulp (8 significand bits) at the exponent of x, with the subnormal floor (ulp 2^-133)"""
    _, e = torch.frexp(x.double())                             # |x| = m 2^e, 0.5 <= m < 1: ulp = 2^(e - 8)
    return torch.pow(2.0, (e.double() - 9.0).clamp_min(-134.0)).to(torch.float64)


def merge_bound(exact: torch.Tensor, mag: torch.Tensor, adapters) -> torch.Tensor:
    sum_r = sum(int(a.shape[0]) for a, _, _ in adapters)
    return half_ulp_bf16(exact) + 2.0 * (sum_r + len(adapters) + 2) * 2.0 ** -24 * mag


def assert_merged(out: torch.Tensor, w: torch.Tensor, adapters, what: str) -> None:
    exact, mag = lora_merge_f64(w, adapters)
    err = (out.double().cpu() - exact).abs()
    bound = merge_bound(exact, mag, adapters)
    bad = err > bound
    worst = float((err / bound).max())
    print(f"{what}: max err / bound {worst:.4f}")
    assert out.dtype == BF and not bool(bad.any()), f"{what}: {int(bad.sum())} of {bad.numel()} elements beyond the bound (worst {worst:.3f} x)"


def naive_merge(w: torch.Tensor, adapters) -> torch.Tensor:
    """the merge that is NOT wanted: every adapter's delta rounded to bf16 before it is added (what `W += (s B A).bfloat16()` does)"""
    out = w.float().cpu()
    for a, b, s in adapters:
        out = (out + (float(s) * (b.double().cpu() @ a.double().cpu())).to(BF).float()).to(BF).float()
    return out.to(BF)


def violates(out: torch.Tensor, w: torch.Tensor, adapters) -> bool:
    exact, mag = lora_merge_f64(w, adapters)
    return bool(((out.double().cpu() - exact).abs() > merge_bound(exact, mag, adapters)).any())
