"""Record tests/golden/attention_launch_shapes.json: what the host-side launch selection of the flash attention answers for a
sweep of call shapes -- osk_attention_launch_shape (key parts of the tail units, query rows per work unit),
osk_attention_tail_split_factor and osk_attention_body_name.  No GPU: without a device the library assumes 256 CUs, and the
fixture is recorded (and checked, tests/test_attention_entry_host.py) under that assumption.

    python tools/make_golden_attention_launch_shapes.py

Record it from the library whose selection is the reference: OSK_ALT_LIB=<path to its libosk_hip.so> (tools/_altlib.py) picks
another build than the tree's.  The fixture holds numbers and kernel names only.
"""
from __future__ import annotations

import itertools
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools import _altlib  # noqa: E402

_altlib.install()
from open_sora_amd import _C  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "attention_launch_shapes.json")
GRID = {
    "hd": [64, 72, 128],
    "B": [1, 2, 3, 6],
    "H": [2, 16, 17],
    "Lq": [130, 1024, 2048, 8448, 16896],
    "segments": [[1, 64], [1, 1000], [1, 16896], [2, 100], [3, 192], [4, 203]],   # (n_seg, seg_len)
    "bound": [0.0, 12.9, 56.0, 300.0],
    "workspace": [0, 1],   # none / osk_attention_workspace_bytes()
}
# every STRIDE-th tuple of the full product (8640): a few hundred calls.  17 is coprime to the 48 (segments, bound, workspace)
# combinations that vary fastest, so all of them -- and every value of the slower axes -- are met
STRIDE = 17


def main() -> None:
    lib = _C.lib
    assert not _C.torch.cuda.is_available(), "record without a device (256 CUs assumed), as the test runs"
    ws_bytes = int(lib.osk_attention_workspace_bytes())
    shapes = []
    for hd, B, H, Lq, (n_seg, seg_len), bound, ws in list(itertools.product(*GRID.values()))[::STRIDE]:
        nbytes = ws * ws_bytes
        parts, rows = _C.attention_launch_shape(B, H, Lq, n_seg, seg_len, hd, bound, nbytes)
        split = int(lib.osk_attention_tail_split_factor(B, H, Lq, n_seg, seg_len, hd, nbytes))
        shapes.append([hd, B, H, Lq, n_seg, seg_len, bound, ws, parts, rows, split])
    bodies = [[hd, n_seg, seg_len, bound, _C.attention_body(hd, n_seg, seg_len, bound)]
              for hd, (n_seg, seg_len), bound in itertools.product(GRID["hd"], GRID["segments"], GRID["bound"])]
    with open(OUT, "w") as f:
        f.write('{"grid": %s,\n "workspace_bytes": %d,\n' % (json.dumps(GRID), ws_bytes))
        f.write(' "shape_columns": ["hd", "B", "H", "Lq", "n_seg", "seg_len", "bound", "workspace", "parts", "rows", "split_factor"],\n')
        f.write(' "shapes": [\n' + ",\n".join("  " + json.dumps(r) for r in shapes) + "],\n")
        f.write(' "body_columns": ["hd", "n_seg", "seg_len", "bound", "body"],\n')
        f.write(' "bodies": [\n' + ",\n".join("  " + json.dumps(r) for r in bodies) + "]}\n")
    print(f"wrote {OUT}: {len(shapes)} launch shapes, {len(bodies)} bodies, {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
