"""
Record the two fixtures that hold the engine's host layer in place while it is rewritten (tests/engine_routes.py lists the routes):

    python tests/golden/make_golden_engine_calls.py host [OUT]     # tests/golden/engine_call_args.json, no GPU
    python tests/golden/make_golden_engine_calls.py gpu [OUT]      # tests/golden/engine_routes_bits.npz, on a GPU box

host: for every HipEngine route the ordered C calls with their arguments, what the route returns from outputs filled by a stand-in
library, and the type and text of every refusal (tests/test_engine_calls_host.py).  gpu: every numeric result of the same routes and
of the public pricer functions over them at 1 000 paths, bit for bit, and per route the kernel names the engine's timer reports
(tests/test_gpu_engine_routes_bits.py).  The library is the one the package loads (SVMC_LIB, SVMC_EXT_LIB and SVMC_EST_LIB name
other builds); nothing outside the repository is read.

Both were recorded on commit 52c9ed2 ("Full-launch LogSV stepping draws one pair of normals ahead"), the parent of the change that
gave the chain entries one call path and the hosts one step grid.  They are this project's own output and are never regenerated
from the code they test: a later change of the ABI records its new routes on ITS parent.
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if "stochvolmodels_amd" not in sys.modules:         # (a caller may have imported another checkout of the package first)
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
HOST_FIXTURE = os.path.join(HERE, "engine_call_args.json")
GPU_FIXTURE = os.path.join(HERE, "engine_routes_bits.npz")


def main(argv):
    import engine_routes
    mode = argv[1] if len(argv) > 1 else ""
    if mode == "host":
        target = argv[2] if len(argv) > 2 else HOST_FIXTURE
        rec = engine_routes.record_host()
        with open(target, "w") as fh:
            fh.write("{\n" + ",\n".join(
                json.dumps(group) + ": {\n" + ",\n".join(json.dumps(k) + ": " + json.dumps(v) for k, v in routes.items()) + "\n}"
                for group, routes in rec.items()) + "\n}\n")
        print(f"{sum(len(v) for v in rec.values())} routes -> {target}")
    elif mode == "gpu":
        target = argv[2] if len(argv) > 2 else GPU_FIXTURE
        arrays, notes = engine_routes.run_gpu()
        np.savez_compressed(target, __notes__=np.array(json.dumps(notes)), **arrays)
        print(f"{len(notes)} routes, {len(arrays)} arrays -> {target}")
    else:
        raise SystemExit(__doc__)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
