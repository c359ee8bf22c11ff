"""
Generate tests/golden/mgf_slice_bits.npz: inputs of the five transform-inversion slice kernels (mgf_vanilla_slice_kernel,
mgf_qvar_slice_kernel, mgf_gamma_slice_kernel, mgf_pdf_slice_kernel, mgf_digital_slice_kernel) and the doubles their C entry
points wrote for them, which tests/test_gpu_transform_odes.py::test_slice_kernels_bit_equal_to_recorded replays bit for bit.
Needs a GPU, and records whatever library is loaded: it is run ONCE, with the library of the commit BEFORE a change that must
not move a bit (built into a directory of its own and selected with SVMC_LIB), never again with the changed one.

    SVMC_LIB=/path/to/the/earlier/libsvmc.so python tests/golden/make_golden_mgf_slice_bits.py [--out FILE]

Shapes -- the smallest at which the shared sum loop, the reduction tree or the chunking can go wrong:
  n_grid 3, 256, 257, 1001   one thread active, exactly one trip of the 256-thread stride loop, a ragged second trip, four trips
  33 strikes                 a full 32-strike chunk plus one (vanilla, qvar, gamma, digital)
  3 sets                     vanilla, digital, gamma (one shortcut set, two complex-weight sets, calls and puts); qvar has one
  65 sets, 2 space points    pdf: across the 64-set launch boundary, every third scale negative
  both weight rules for pdf and digital, both contours for digital
  n = 257                    log E of every set has a NaN (point 5) and a -inf (point 256, the second trip), the third set a
                             +inf (point 200) as well; qvar runs on the first and on the third set
The grids are synthetic_grid / density_grid of the test module (the third set's is stretched, so the local-step weights
differ point to point); a case names the rows it takes, so the 65 pdf sets share three stored grids.
"""
import argparse
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import test_gpu_transform_odes as T  # noqa: E402

NS = (3, 256, 257, 1001)
SCALERS = (0.16, 0.05, 0.3)
K = 33


def base_grids(n):
    grids = [T.synthetic_grid(n, SCALERS[0], seed=0), T.synthetic_grid(n, SCALERS[1], seed=1),
             T.density_grid(n, SCALERS[2], True, 2, 0)]
    p, lm = np.stack([g[0].imag for g in grids]), np.stack([g[1] for g in grids])
    if n == 257:
        lm[:, 5] = complex(np.nan, 0.0)
        lm[:, 256] = complex(-np.inf, 0.0)
        lm[2, 200] = complex(np.inf, 0.0)
    return p, lm


def build_cases():
    arrays, index = {}, []
    for n in NS:
        arrays[f"p_{n}"], arrays[f"lm_{n}"] = base_grids(n)

    def add(kernel, n, tag, sets, re, scalars, **small):
        cid = f"{kernel}_n{n}{tag}"
        index.append({"id": cid, "kernel": kernel, "n": n, **scalars})
        arrays[cid + "/sets"] = np.asarray(sets, dtype=np.int64)
        arrays[cid + "/re"] = np.asarray(re, dtype=np.float64)
        for name, v in small.items():
            arrays[cid + "/" + name] = v

    three = [0, 1, 2]
    for n in NS:
        forward = 1.3
        strikes = forward * np.exp(np.linspace(-0.6, 0.6, K))
        add("vanilla", n, "", three, [-0.5, -0.5, 0.5], {"forward": forward}, strikes=strikes)
        for row in ([0], [2]) if n == 257 else ([0],):
            add("qvar", n, f"_set{row[0]}", row, [-0.5], {"ttm": 0.5}, strikes=np.linspace(0.05, 2.0, K))
        gammas = np.array([-1.0, 0.7, -0.2])
        add("gamma", n, "", three, [0.5 + gammas[0], -0.5, -0.1], {"forward": 1.1}, strikes=1.1 * np.exp(np.linspace(-0.5, 0.5, K)),
            gammas=gammas, shortcut=np.array([1, 0, 0], dtype=np.int32), codes=(np.arange(K) % 2).astype(np.int32),
            normalizers=np.array([1.0, 0.97, 1.04]), gamma_forwards=np.array([1.1, 1.08, 1.13]))
        for is_simpson in (1, 0):
            for negative_contour in (1, 0):
                add("digital", n, f"_simpson{is_simpson}_neg{negative_contour}", three, [-0.5 if negative_contour else 0.5] * 3,
                    {"forward": forward, "negative_contour": negative_contour, "is_simpson": is_simpson}, strikes=strikes)
            sets = np.arange(65) % 3
            i = np.arange(65)
            scales = np.where(i % 3 == 1, -1.0, 1.0) * np.take(SCALERS, sets) * (1.5 + 0.1 * (i % 5))
            shifts = 0.01 * (i % 7) - 0.02
            space = shifts[:, None] + np.abs(scales)[:, None] * np.array([-1.5, 1.0])[None, :] * (1.0 + 0.01 * i[:, None])
            add("pdf", n, f"_simpson{is_simpson}", sets, np.where(i % 2 == 0, -0.5, 0.5), {"is_simpson": is_simpson},
                space=np.ascontiguousarray(space), shifts=shifts, scales=scales)
    arrays["index"] = np.array(json.dumps(index))
    return arrays, index


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "mgf_slice_bits.npz"))
    args = ap.parse_args()
    from stochvolmodels_amd import _lib
    L = _lib.load()
    arrays, index = build_cases()
    for c in index:
        arrays[c["id"] + "/out"] = T.slice_case_output(L, arrays, c)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    np.savez_compressed(args.out, **arrays)
    print("library", _lib.LIB_PATH)
    print("wrote", args.out, os.path.getsize(args.out), "bytes,", len(index), "cases")


if __name__ == "__main__":
    main()
