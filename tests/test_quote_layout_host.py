"""
The workspace, image and page-locked layouts of the four quote-table tails and their image builders (csrc/svmc_quotes.h) on the
host, with no GPU: tests/native/quote_layout_probe.cpp is compiled with g++ -- the header includes no HIP header -- and run.  The
program makes the assertions (its head comment lists them); this test adds that the four workspace sizes it measures at the bound
the public size functions use are the ones recorded from the library in tests/golden/quote_tails.npz.
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "native", "quote_layout_probe.cpp")
GOLDEN = os.path.join(ROOT, "tests", "golden", "quote_tails.npz")
SIZE_N, SIZE_MK, SIZE_P = (1, 256, 257, 300000), ((1, 0), (1, 1), (3, 17), (16, 208)), (1, 6, 31)     # make_golden_quote_tails.py's grid


@pytest.fixture(scope="module")
def probe_output(tmp_path_factory):
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to compile the host probe"
    exe = str(tmp_path_factory.mktemp("quote_layout") / "quote_layout_probe")
    subprocess.run([gxx, "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
                    "-I" + os.path.join(ROOT, "stochvolmodels_amd", "csrc"), SOURCE, "-o", exe], check=True)
    res = subprocess.run([exe], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    return res.stdout.splitlines()


def test_every_layout_and_image_builder_passes_the_probes_assertions(probe_output):
    assert probe_output[-1] == "ok"
    sizes = [line for line in probe_output if line.startswith("size ")]
    assert len(sizes) == 5 * 3 * 4                      # five chains (the grid's four and 16 ragged expiries) x P x n_path


def test_the_measured_workspace_sizes_are_the_recorded_ones(probe_output):
    recorded = np.load(GOLDEN, allow_pickle=False)["sizes"]
    measured = {}
    for line in probe_output:
        if line.startswith("size "):
            n, m, k, p, *four = (int(v) for v in line.split()[1:])
            measured[(n, m, k, p)] = four
    for i, n in enumerate(SIZE_N):
        for j, (m, k) in enumerate(SIZE_MK):
            for q, p in enumerate(SIZE_P):
                assert measured[(n, m, k, p)] == recorded[i, j, q, :4].tolist(), (n, m, k, p)
