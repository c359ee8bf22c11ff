"""
The data behind Fig. 6 of "Log-normal stochastic volatility model with quadratic drift" (the reference's
papers/logsv_model_with_quadratic_drift/article_figures.py:82-146, plot_var_pdfs, minus the plotting): for the log-return, the
annualised quadratic variance and the volatility, the first- and second-order model densities on a 200-point space grid beside
the histogram of 400 000 simulated terminal values.  Prints each table's column sums, as the reference's script does.

    python examples/density_figure.py [--ttm 0.0833] [--nb-path 400000] [--device-histogram] [--device-kde]

--device-histogram counts on the GPU (LogSVPricer.terminal_value_histograms) instead of downloading the three state vectors.
--device-kde adds the Gaussian kernel estimate of the same paths (scipy.stats.gaussian_kde's, summed on the GPU by
engine_state_kdes from the state the simulation left there) as bin masses, density x dx, beside the histogram.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import pandas as pd  # noqa: E402

from stochvolmodels_amd import ExpansionOrder, LogSvParams, LogSVPricer, VariableType  # noqa: E402
from stochvolmodels_amd.engine import get_engine  # noqa: E402
from stochvolmodels_amd.pricers.logsv_pricer import engine_state_kdes  # noqa: E402
from stochvolmodels_amd.utils.funcs import compute_histogram_data, set_seed  # noqa: E402


def var_pdfs(params: LogSvParams, ttm: float = 1.0, n: int = 200, vol_scaler: float = None, nb_path: int = 400000,
             device_histogram: bool = False, device_kde: bool = False) -> dict:
    logsv_pricer = LogSVPricer()
    names = {VariableType.LOG_RETURN: "Log-return X", VariableType.Q_VAR: "Quadratic variance I / ttm",
             VariableType.SIGMA: "Volatility sigma"}
    grids = {vt: params.get_variable_space_grid(variable_type=vt, ttm=ttm, n=n, n_stdevs=4.5) for vt in names}
    if device_histogram:
        mcs = logsv_pricer.terminal_value_histograms(params=params, ttm=ttm, nb_path=nb_path, space_grids=grids)
    else:
        x0, sigma0, qvar0 = logsv_pricer.simulate_terminal_values(ttm=ttm, params=params, nb_path=nb_path)
        datas = {VariableType.LOG_RETURN: x0, VariableType.Q_VAR: qvar0 / ttm, VariableType.SIGMA: sigma0}
        mcs = {vt: compute_histogram_data(data=datas[vt], x_grid=grids[vt], name="MC") for vt in names}
    # the terminal state of the simulation above is still resident on its engine
    kdes = engine_state_kdes(get_engine(nb_path), grids, ttm) if device_kde else {}
    out = {}
    for variable_type, title in names.items():
        space_grid = grids[variable_type]
        xpdf1 = logsv_pricer.logsv_pdfs(params=params, ttm=ttm, space_grid=space_grid, variable_type=variable_type,
                                        expansion_order=ExpansionOrder.FIRST, vol_scaler=vol_scaler, is_stiff_solver=True)
        xpdf2 = logsv_pricer.logsv_pdfs(params=params, ttm=ttm, space_grid=space_grid, variable_type=variable_type,
                                        expansion_order=ExpansionOrder.SECOND, vol_scaler=vol_scaler, is_stiff_solver=True)
        kde = [pd.Series(kdes[variable_type][0] * (space_grid[1] - space_grid[0]), index=space_grid, name="MC kernel estimate")] \
            if device_kde else []
        df = pd.concat([mcs[variable_type].rename("MC")] + kde + [pd.Series(xpdf1, index=space_grid, name="1st order Expansion"),
                        pd.Series(xpdf2, index=space_grid, name="2nd order Expansion")], axis=1)
        print(title)
        print(df.sum(axis=0))
        out[variable_type] = df
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--ttm", type=float, default=1.0 / 12.0)
    ap.add_argument("--nb-path", type=int, default=400000)
    ap.add_argument("--device-histogram", action="store_true")
    ap.add_argument("--device-kde", action="store_true")
    args = ap.parse_args()
    set_seed(37)
    np.set_printoptions(precision=6)
    # the parameters and maturity of the article's figure (article_figures.py:276-287); vol_scaler=None: the grid scale follows
    # sigma0 and ttm instead of the option chain the article's script loads
    var_pdfs(LogSvParams(sigma0=0.4083, theta=0.3789, kappa1=2.21, kappa2=2.18, beta=0.5010, volvol=0.6 * 3.0633), ttm=args.ttm,
             nb_path=args.nb_path, device_histogram=args.device_histogram, device_kde=args.device_kde)
