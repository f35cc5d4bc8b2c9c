"""CPU: the oracle restatement against what the reference's own MMDiTModel returned, fp32 and bf16, on the same synthetic
weights and inputs (recorded in tests/golden/ref_checks.npz by oracle/make_golden_refchecks.py)."""
import os

import numpy as np
import pytest
import torch

from oracle import configs, mmdit_oracle as O
from tests import ref_cases as R
from tests.util import rel_l2, torch_inputs, torch_params

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_checks.npz")


@pytest.mark.parametrize("name", ["hd64_eager_fused", "hd72_liger_fused", "hd128_liger_split"])
def test_forward_fp32_and_bf16(name):
    assert name in R.MMDIT_NAMES
    cfg, B, T, h, w, L_txt = configs.GOLDEN[name]
    g = np.load(GOLDEN)
    sd = torch_params(cfg)
    inp = torch_inputs(cfg, B, T, h, w, L_txt)
    ref = torch.from_numpy(g[f"mmdit_{name}_fp32"])
    with torch.inference_mode():
        mine = O.forward(sd, cfg, **inp)
    assert ref.shape == mine.shape
    assert (ref - mine).abs().max() <= 2e-5 * max(float(ref.abs().max()), 1.0)
    # bf16: same rounding points -> both sit at the same distance from the fp32 truth
    sdb = {k: v.bfloat16() for k, v in sd.items()}
    inpb = torch_inputs(cfg, B, T, h, w, L_txt, dtype=torch.bfloat16)
    refb = torch.from_numpy(g[f"mmdit_{name}_bf16"])
    with torch.inference_mode():
        mineb = O.forward(sdb, cfg, **inpb).float()
    e_ref, e_mine = rel_l2(refb, ref), rel_l2(mineb, ref)
    assert e_mine <= 1.5 * e_ref and e_ref <= 1.5 * e_mine, (e_ref, e_mine)


def test_reference_error_conventions():
    """ValueError for ndim != 3 / missing cond (model.py:172-179) are mirrored by the oracle."""
    cfg, B, T, h, w, L_txt = configs.GOLDEN["hd64_eager_fused"]
    sd = torch_params(cfg)
    inp = torch_inputs(cfg, B, T, h, w, L_txt)
    bad = dict(inp)
    bad["img"] = inp["img"][0]
    with pytest.raises(ValueError):
        O.forward(sd, cfg, **bad)
    bad = dict(inp)
    bad.pop("cond")
    with pytest.raises(ValueError):
        O.forward(sd, cfg, **bad)
