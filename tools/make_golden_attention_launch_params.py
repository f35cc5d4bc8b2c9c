"""Record tests/golden/attention_launch_params.json: the launches every flash-attention entry point makes for a set of well-formed
calls, and every AttnParams field of each launch.  tests/attention_param_probe.hip is a stand-alone host program: it compiles
open_sora_amd/csrc/attention_fwd.hip against stub launch functions that record their parameter block (no kernel runs, no GPU is
asked for anything; 256 CUs assumed) and prints one JSON object per call.

    python tools/make_golden_attention_launch_params.py

Record it from the attention_fwd.hip whose launches are the reference: the fixture pins what a host-side change must not move.
tests/test_attention_entry_host.py builds the probe the same way and compares field for field.  The fixture holds numbers, kernel
names and argument-relative offsets only.
"""
from __future__ import annotations

import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from open_sora_amd import build  # noqa: E402

SRC = os.path.join(ROOT, "tests", "attention_param_probe.hip")
OUT = os.path.join(ROOT, "tests", "golden", "attention_launch_params.json")


def build_probe(out_dir: str) -> str:
    """compile the probe (one translation unit: it includes attention_fwd.hip) with the library's flags; returns the program's path"""
    exe = os.path.join(out_dir, "attention_param_probe")
    r = subprocess.run([build._hipcc(), *build.flags_for(SRC), SRC, "-o", exe], capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"hipcc failed on {os.path.basename(SRC)} ({r.returncode}):\n{r.stderr[-4000:]}")
    return exe


def run_probe(exe: str) -> dict:
    """{"fields": [...], "calls": [{"call", "status", "launches": [[field values]]}]} as the program prints it"""
    r = subprocess.run([exe], capture_output=True, text=True, check=True)
    head, *calls = [json.loads(o) for o in r.stdout.replace("\n  ", " ").splitlines()]
    return {"fields": head["fields"], "calls": calls}


def main() -> None:
    import tempfile

    with tempfile.TemporaryDirectory() as d:
        got = run_probe(build_probe(d))
    with open(OUT, "w") as f:
        f.write('{"fields": %s,\n "calls": [\n' % json.dumps(got["fields"]))
        f.write(",\n".join('  {"call": %s, "status": %d, "launches": [\n%s]}' %
                           (json.dumps(c["call"]), c["status"], ",\n".join("    " + json.dumps(row) for row in c["launches"]))
                           for c in got["calls"]))
        f.write("]}\n")
    print(f"wrote {OUT}: {len(got['calls'])} calls, {sum(len(c['launches']) for c in got['calls'])} launches, {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
