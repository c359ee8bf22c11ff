"""
Many independent LogSV / Heston jobs of one chain in one call (svmc_logsv_chain_price_many, svmc_heston_chain_price_many,
logsv_mc_chain_pricer_many, heston_mc_chain_pricer_many): what holds without a GPU -- the library exports the two entry
points the header declares, the Python names exist, and the argument checks come before any device work.
"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("svmc_logsv_chain_price_many", "svmc_heston_chain_price_many")


def _chain():
    ttms = np.array([1 / 12, 0.25])
    strikes = [np.linspace(0.9, 1.1, 3), np.linspace(0.8, 1.2, 3)]
    types = [np.array(["P", "C", "C"]), np.array(["P", "C", "C"])]
    return dict(ttms=ttms, forwards=np.ones(2), discfactors=np.ones(2), strikes_ttms=strikes, optiontypes_ttms=types)


def test_library_exports_and_header_declares_the_many_entry_points():
    from stochvolmodels_amd import build
    lib = build.build()
    exported = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    header = open(os.path.join(ROOT, "include", "svmc.h")).read()
    for name in NAMES:
        assert re.search(r"\bT " + name + r"\b", exported), name
        assert re.search(r"SVMC_API\s+int\s+" + name + r"\s*\(", header), name
    assert int(re.search(r"#define SVMC_MANY_MAX_JOBS (\d+)", header).group(1)) >= 1


def test_binding_declares_the_many_entry_points():
    from stochvolmodels_amd import _lib
    L = _lib.load()
    for name in NAMES:
        assert name in L._svmc_symbols
        assert len(getattr(L, name).argtypes) == 17


def test_job_cap_is_one_number():
    from stochvolmodels_amd.engine import MANY_MAX_JOBS
    header = open(os.path.join(ROOT, "include", "svmc.h")).read()
    assert MANY_MAX_JOBS == int(re.search(r"#define SVMC_MANY_MAX_JOBS (\d+)", header).group(1))


def test_python_names_exist():
    import stochvolmodels_amd as sv
    from stochvolmodels_amd.pricers import heston_pricer, logsv_pricer
    assert sv.logsv_mc_chain_pricer_many is logsv_pricer.logsv_mc_chain_pricer_many
    assert sv.heston_mc_chain_pricer_many is heston_pricer.heston_mc_chain_pricer_many
    assert callable(sv.LogSVPricer.model_mc_price_chain_many)
    assert callable(sv.HestonPricer.model_mc_price_chain_many)


def test_seed_count_mismatch_raises_before_device_work():
    import stochvolmodels_amd as sv
    from stochvolmodels_amd.utils.funcs import get_rng_state
    before = get_rng_state()
    lp = [sv.LOGSV_BTC_PARAMS, sv.LOGSV_BTC_PARAMS]
    with pytest.raises(ValueError):
        sv.logsv_mc_chain_pricer_many(lp, seeds=[1], **_chain())
    with pytest.raises(ValueError):
        sv.heston_mc_chain_pricer_many([sv.HestonParams()], seeds=[1, 2], **_chain())
    chain = sv.OptionChain(ids=None, **_chain())
    with pytest.raises(ValueError):
        sv.LogSVPricer().model_mc_price_chain_many(chain, lp, seeds=[3, 4, 5])
    with pytest.raises(ValueError):
        sv.HestonPricer().model_mc_price_chain_many(chain, [sv.HestonParams()], seeds=[])
    assert get_rng_state() == before          # no call id taken


def test_empty_list_returns_empty_without_device_work():
    import stochvolmodels_amd as sv
    from stochvolmodels_amd.utils.funcs import get_rng_state
    before = get_rng_state()
    assert sv.logsv_mc_chain_pricer_many([], **_chain()) == []
    assert sv.heston_mc_chain_pricer_many([], seeds=[], **_chain()) == []
    assert get_rng_state() == before


def test_c_example_compiles_and_links(tmp_path):
    """examples/price_chain_many.c is a plain-C host of the new entry points (run by tests/test_gpu_mc_many.py)"""
    from stochvolmodels_amd import build
    lib = build.build()
    exe = str(tmp_path / "price_chain_many")
    libdir = os.path.dirname(lib)
    subprocess.run(["gcc", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "examples", "price_chain_many.c"), "-o", exe, "-L" + libdir, "-lsvmc",
                    "-Wl,-rpath," + libdir, "-Wl,-rpath-link,/opt/rocm/lib", "-lm"], check=True)
    assert os.path.exists(exe)
