"""oracle/sampling_oracle.py (the CPU restatement of the sampling loop that the GPU tests compare against) pinned to
what the reference's OWN source text returns: I2VDenoiser.denoise, get_schedule, pack, unpack of opensora/utils/sampling.py,
recorded by oracle/make_golden_refchecks.py on the seeded inputs of tests/ref_cases.py in tests/golden/ref_checks.npz.  CPU only."""
import os

import numpy as np
import pytest
import torch

from oracle import sampling_oracle as S
from tests import ref_cases as R

BF = torch.bfloat16
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_checks.npz")


@pytest.fixture(scope="module")
def ref():
    return np.load(GOLDEN)


def test_schedule_pack_unpack_match_the_reference(ref):
    for i, (n, L, T, kw) in enumerate(R.SCHEDULES):
        assert S.schedule(n, L, T, **kw) == ref[f"schedule_{i}"].tolist()
    z = R.pack_input()
    assert torch.equal(S.pack(z), torch.from_numpy(ref["pack"]))
    assert torch.equal(S.unpack(S.pack(z), 4, 6, 3), z)
    assert torch.equal(torch.from_numpy(ref["unpack"]), z)


@pytest.mark.parametrize("dtype", [torch.float32, BF])
@pytest.mark.parametrize("osci", [False, True])
def test_i2v_denoise_is_the_reference_loop_bit_for_bit(ref, dtype, osci):
    """same stub model, same inputs: the restated loop equals I2VDenoiser.denoise exactly, in fp32 and in bf16
    (same operations in the same order and dtype)."""
    model, z, masks, masked_ref, sched = R.i2v_case(dtype)
    kw = dict(text_osci=osci, image_osci=osci, scale_temporal_osci=osci)
    want = torch.from_numpy(ref[R.i2v_key(dtype, osci)]).to(dtype)
    got = S.i2v_denoise(model, S.pack(z).repeat(3, 1, 1), S.schedule(*sched), 7.5, 3.0, masks, masked_ref, **kw)
    assert got.dtype == want.dtype and torch.equal(got, want)
