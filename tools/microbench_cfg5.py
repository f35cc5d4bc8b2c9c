#!/usr/bin/env python
"""Per-rank kernel times of BASELINE configs[4] (11B geometry, 64 x 720p latent read as T_lat = 64: L = 230,912 tokens, SP = 8; bf16 and
the fp8 mode) measured on ONE GPU, with the loop bodies the model selects there (bounded FAST body in bf16, the fp8 P.V body in fp8 mode)
-- a thin wrapper of tools/rank_shapes.py (round 6: the earlier version timed the general body; see microbench_cfg4.py).
--qk8: instead, the A/B of osk_attention_fwd_pv8_bf16 against osk_attention_fwd_qk8_bf16 (rank_shapes.attention_qk8_ab)."""
import json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from tools import rank_shapes

if "--qk8" in sys.argv:   # the fp8-QK^T attention against the pv8 one at the 11B bench shape and the configs[4] rank shape (one JSON line each)
    for name in rank_shapes.QK8_SHAPES:
        print(json.dumps({"qk8_ab": name, **rank_shapes.attention_qk8_ab(torch.device("cuda", 0), name)}), flush=True)
else:
    print(json.dumps(rank_shapes.measure(torch.device("cuda", 0), ("cfg4",))["cfg4"]), flush=True)
