"""One fixed sequence of calls that reaches every kind of step graph and both rollback paths, for
counting launches per kernel name between two builds of the library (GPK_LIB_PATH selects it):

    rocprofv3 --kernel-trace --stats -d OUT -- python tools/step_graph_scenario.py

Handle 1 (C4): prepare(150), step(150), step(22), step(13), 5 x step(1), loss_grad() -- prepared
whole-chunk and plain batch graphs, the 8-step and single-step graphs, the one-step call graph and
the apply = 0 graph.  Handle 2 (tests' 2d_open case, GPK_FLAG_FAST_FIRST): step(4), step(1) -- a
fast batch that meets an open gate, restored and rerun on the full graph.  Prints the losses'
checksum, so that two runs can also be told to have computed the same thing.
"""
import os
import sys
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "gaussian-process-slover-for-high-freq-pde_amd")]
import numpy as np  # noqa: E402
from gpk._lib import GPK_FLAG_FAST_FIRST  # noqa: E402
from gpk.problems import make_solver  # noqa: E402
from tests.helpers import device_solver, problem_2d  # noqa: E402


def main():
    out = []
    s = make_solver("C4", seed=0)
    try:
        s.prepare(150)
        out += [s.step(150), s.step(22), s.step(13)]
        out += [s.step(1) for _ in range(5)]
        loss, grad = s.loss_grad()
        out += [[loss], grad]
        modes = [s.graph_mode()]
    finally:
        s.close()
    prob, params, _, fs = problem_2d(eq="allencahn", kind="Matern52_1d", n1=40, n2=36, Q=5, seed=4)
    s = device_solver(prob, 5, fs, flags=GPK_FLAG_FAST_FIRST)
    try:
        s.set_params(params)
        out += [s.step(4), s.step(1)]
        s.sync()
        modes.append(s.graph_mode())
    finally:
        s.close()
    flat = np.concatenate([np.asarray(x, dtype=np.float64).reshape(-1) for x in out])
    print(f"values {flat.size} crc32 {zlib.crc32(flat.tobytes()):08x} graph_mode {modes}")


if __name__ == "__main__":
    main()
