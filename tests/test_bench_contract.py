"""Host-side pieces of bench.py that do not need a GPU: the command-line contract of the driver
(`python bench.py --gpus N --steps K --warmup W`, defaults = N 1 and a K / W that finish within minutes), the self-spawn of
`--gpus N > 1` (one rank per GPU under torch.distributed.run, rendezvous on 127.0.0.1) and the committed profile records the
bench line reads its `roofline.traffic` from."""
import importlib.util
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_defaults_and_flags(monkeypatch):
    b = _bench()
    monkeypatch.setattr(sys, "argv", ["bench.py"])
    a = b.parse()
    assert (a.gpus, a.workload, a.model, a.cfg_batch, a.fp8) == (1, "dit", "XL", 3, False)
    assert 1 <= a.warmup <= a.steps <= 20          # the default run must finish within minutes
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "8", "--steps", "5", "--warmup", "2"])
    a = b.parse()
    assert (a.gpus, a.steps, a.warmup) == (8, 5, 2)
    assert b.SAMPLING_STEPS == 30 and b.MFMA_BF16_PEAK_TFLOPS == 2500.0
    assert a.full is False and a.dump_outputs is None      # a plain run times the headline only
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "out_dir"])
    a = b.parse()
    assert a.full is True and a.dump_outputs == "out_dir"


def test_dump_outputs_writes_float32_npy(tmp_path):
    import numpy as np
    import torch

    b = _bench()
    x = torch.randn(1, 40, 64, generator=torch.Generator().manual_seed(0)).to(torch.bfloat16)
    b.dump_outputs(str(tmp_path / "d"), {"latents": x})
    a = np.load(tmp_path / "d" / "latents.npy")
    assert a.dtype == np.float32 and a.shape == (1, 40, 64) and np.array_equal(a, x.float().numpy())
    # over the size limit: a fixed sample of each array, the same positions in every run, nothing larger than the limit
    y = torch.randn(3, 1000, generator=torch.Generator().manual_seed(1))
    for d in ("s1", "s2"):
        b.dump_outputs(str(tmp_path / d), {"latents": x, "video": y}, limit_bytes=4000)
    s1 = {n: np.load(tmp_path / "s1" / f"{n}.npy") for n in ("latents", "video")}
    s2 = {n: np.load(tmp_path / "s2" / f"{n}.npy") for n in ("latents", "video")}
    assert all(np.array_equal(s1[n], s2[n]) and s1[n].dtype == np.float32 for n in s1)
    assert sum(v.nbytes for v in s1.values()) <= 4000 and set(s1["video"].tolist()) <= set(y.reshape(-1).tolist())


def test_self_spawn_uses_one_rank_per_gpu_on_localhost(monkeypatch):
    b = _bench()
    seen = {}
    import subprocess

    monkeypatch.setattr(subprocess, "call", lambda cmd: seen.setdefault("cmd", cmd) and 0)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "4", "--steps", "3"])
    assert b._self_spawn(4) == 0
    cmd = seen["cmd"]
    assert cmd[1:3] == ["-m", "torch.distributed.run"] and "--nnodes=1" in cmd and "--nproc-per-node=4" in cmd
    assert cmd[cmd.index("--master-addr") + 1] == "127.0.0.1" and int(cmd[cmd.index("--master-port") + 1]) > 0
    assert cmd[-4:] == ["--gpus", "4", "--steps", "3"] and os.path.basename(cmd[-5]) == "bench.py"


def test_traffic_records_the_bench_line_cites_exist():
    recs = json.load(open(os.path.join(ROOT, "profiles", "kernel_traffic.json")))
    conv = [r for r in recs if r["kernel"].startswith("conv256")]
    assert conv and all(os.path.exists(os.path.join(ROOT, r["source"])) for r in recs)
    assert conv[-1]["hbm_bytes_per_step"] == int(conv[-1]["fetch_size_kb"] * 1024 * 2 + conv[-1]["write_size_kb"] * 1024)
    attn = json.load(open(os.path.join(ROOT, "profiles", "attn_traffic.json")))
    assert any(r["kernel"] == "attn_asm72_kernel" and r["shape"] == [3, 16, 16896, 72] and
               os.path.exists(os.path.join(ROOT, r["source"])) for r in attn)
