"""Child process of tests/test_gpu_bound_overlap.py: ABO_TAIL32_STAGE is read once per process, so each setting
of it runs in a process of its own — this one, with the setting in its environment.  Runs every case of CASES through the pruned
selection with a first bound level of 256 rows (fused fp32 head, fp32 tail) and writes, per case, the selection, the statistics and the
first level's per-candidate outputs to the .npz file named on the command line."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
os.environ["ABO_LIB_TEST_HOOKS"] = "1"

import numpy as np

SF2, NOISE, XI, K, M = 1.0, 1e-3, 0.01, 100, 20000
NEVER = 1 << 40
NAN_ROW = 12345
# name: (N, d, family name, length scale, a NaN coordinate in candidate NAN_ROW)
CASES = {
    "m52_d8": (640, 8, "MATERN52", 1.0, False),
    "se_d8": (640, 8, "SE", 1.0, False),
    "m52_d3": (640, 3, "MATERN52", 0.5, False),
    "se_d3": (640, 3, "SE", 0.5, False),
    "odd_n641": (641, 8, "MATERN52", 1.0, False),
    "odd_n513": (513, 8, "MATERN52", 1.0, False),
    "nan": (640, 8, "MATERN52", 1.0, True),
}


def problem(name):
    from abstractbayesopt.jl_amd import synth
    N, d, fam, ell, nan = CASES[name]
    X, y = synth.standardized_problem(N, d, 0.03)
    Z = synth.points(2, M, d).copy()
    if nan:
        Z[NAN_ROW, 2] = np.nan
    return X, y, Z


def force_first_level(abo):
    """the bound pass forced to 512 rows with a first level of 256 in front, the second level never run: head32 / tail32 over all M"""
    lib = abo._lib.lib()
    abo._lib.check(lib.abo_test_prune_force(2, 0))
    abo._lib.check(lib.abo_test_prune_levels(1, NEVER))


def pruned_call(abo, model, Z, y):
    """→ dict: top_val, top_idx, stats (pruned, bound_rows, level1_rows), mu, eps, head, ssq of the first level"""
    lib = abo._lib.lib()
    acq = abo.ExpectedImprovement(XI, float(np.min(y)))
    _, tv, ti = abo.evaluate(acq, model, Z, k=K, return_scores=False)
    st, lv = model.prune_stats(), model.prune_levels()
    n = Z.shape[0]
    mu, eps, head, ssq = np.empty(n), np.empty(n), np.empty(n), np.empty(n)
    abo._lib.check(lib.abo_test_prune_mean(model._require(), mu.ctypes.data, eps.ctypes.data, n))
    abo._lib.check(lib.abo_test_prune_head(model._require(), head.ctypes.data, ssq.ctypes.data, n))
    return {"top_val": np.asarray(tv, dtype=np.float64), "top_idx": np.asarray(ti, dtype=np.int64),
            "stats": np.array([st["pruned"], st["bound_rows"], lv["level1_rows"]], dtype=np.int64),
            "mu": mu, "eps": eps, "head": head, "ssq": ssq}


def main(out):
    import abstractbayesopt.jl_amd as abo
    from oracle import gp_oracle as O
    from tests.test_gpu_parity import make_model
    force_first_level(abo)
    res = {}
    for name, (N, d, fam, ell, nan) in CASES.items():
        X, y, Z = problem(name)
        model = abo.update(make_model(getattr(O, fam), ell, SF2, NOISE, contraction="int8"), X, y)
        for key, val in pruned_call(abo, model, Z, y).items():
            res[f"{name}.{key}"] = val
    np.savez(out, **res)


if __name__ == "__main__":
    main(sys.argv[1])
