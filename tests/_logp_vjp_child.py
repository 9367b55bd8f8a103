"""Child process of tests/test_gpu_logp.py: the input-gradient-only backward against the training backward on the fused base shape with
the tile-size switches of the environment (they are read once per process).  argv: out path, precision, cells.  Writes
{"equal_dx", "equal_out", "finite"}."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch

from test_gpu_logp import vjp_pair

out, precision, n = sys.argv[1], sys.argv[2], int(sys.argv[3])
y, dx_full, y2, dx = vjp_pair("dit_base", precision, n)
torch.save({"equal_dx": torch.equal(dx, dx_full), "equal_out": torch.equal(y, y2), "finite": bool(torch.isfinite(dx).all()),
            "nonzero": bool(dx.abs().max() > 0)}, out)
