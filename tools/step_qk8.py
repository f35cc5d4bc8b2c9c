#!/usr/bin/env python
"""bench.py's denoise step in fp8 mode with the attention's QK^T on the fp8 MFMA as well: python tools/step_qk8.py [bench.py
arguments, --fp8 among them].  bench.py itself only knows enable_fp8(); here every enable_fp8(True) also asks for qk8, so the same
command with bench.py and with this tool is the A/B of the two fp8 attentions inside the step."""
import os
import runpy
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from open_sora_amd import mmdit

_enable = mmdit.MMDiTModel.enable_fp8
mmdit.MMDiTModel.enable_fp8 = lambda self, on=True, qk8=True: _enable(self, on, qk8=qk8)
sys.argv = [os.path.join(ROOT, "bench.py")] + sys.argv[1:]
runpy.run_path(os.path.join(ROOT, "bench.py"), run_name="__main__")
