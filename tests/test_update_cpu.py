"""CPU tests of update(model, xs, ys) through abo_update / abo_mgpu_update (no GPU needed): the C-ABI is declared, exported and
validates its arguments before touching a device; the incremental_update flag survives every way the driver rebuilds a model;
both Julia shims bind the two entry points with the header's arity and C types."""
import ctypes as C
import os
import pickle
import re

import numpy as np
import pytest

import abstractbayesopt.jl_amd as abo
from tests.test_julia_shim_cpu import SHIMS, c_prototypes, jl_matches_c, julia_calls

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("abo_update", "abo_mgpu_update")


def test_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "abo_hip.h")).read()
    for name in NAMES:
        assert re.search(rf"^int32_t\s+{name}\s*\(", hdr, flags=re.M), name
        assert name in abo._lib.EXPORTS
        assert getattr(abo._lib.lib(), name) is not None
    import subprocess
    for path in (abo._lib.LIB_PATH, abo._lib.LIB_TEST_PATH):
        out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        syms = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
        assert set(NAMES) <= syms, path
    for name, v in (("ABO_UPDATE_SHARED", abo._lib.UPDATE_SHARED), ("ABO_UPDATE_APPENDED", abo._lib.UPDATE_APPENDED),
                    ("ABO_UPDATE_REFIT", abo._lib.UPDATE_REFIT)):
        assert re.search(rf"{name} = {v}\b", hdr), name
    assert re.search(r"#define ABO_ABI_VERSION 7\b", hdr) and "added within ABI 7" in hdr


def test_argument_validation_needs_no_gpu():
    L = abo._lib.lib()
    E = abo._lib.ABO_EINVAL
    prm = abo._lib.AboParams(family=1, device=0, ell=1.0, sigma_f2=1.0, noise_var=1e-3, mean_c=0.0, jitter=0.0)
    X = np.zeros((4, 2))
    y = np.zeros(4)
    out = C.c_void_p()
    info = C.c_int64(7)
    path = C.c_int32(-1)
    fake = C.c_void_p(0x1000)          # never dereferenced: every check below fails before the handle is looked at
    args = lambda **kw: dict(dict(prev=fake, prm=C.byref(prm), X=X.ctypes.data, N=4, d=2, y=y.ctypes.data, space=0, out=C.byref(out)), **kw)

    def call(a):
        return L.abo_update(a["prev"], a["prm"], None, a["X"], a["N"], a["d"], a["y"], a["space"], C.byref(info), C.byref(path), a["out"])

    for bad in (dict(prev=None), dict(prm=None), dict(X=None), dict(y=None), dict(out=None), dict(N=0), dict(N=-3),
                dict(N=(1 << 20) + 1), dict(d=0), dict(d=70000), dict(space=2)):
        info.value, path.value = 7, -1
        assert call(args(**bad)) == E, bad
        assert info.value == 0 and path.value == abo._lib.UPDATE_REFIT
        assert "abo_update" in abo._lib.last_error()
    mg = lambda prev, N=4, d=2, Xp=X.ctypes.data, yp=y.ctypes.data, o=C.byref(out): L.abo_mgpu_update(
        prev, C.byref(prm), None, Xp, N, d, yp, C.byref(info), C.byref(path), o)
    assert mg(None) == E
    for kw in (dict(N=0), dict(d=0), dict(Xp=None), dict(yp=None), dict(o=None)):
        assert mg(fake, **kw) == E, kw
        assert "abo_mgpu_update" in abo._lib.last_error()


@pytest.mark.parametrize("make", [
    lambda: abo.HipStandardGP(abo.Matern52Kernel(), 1e-3, device=0, incremental_update=True),
    lambda: abo.HipGradientGP(abo.Matern52Kernel(), 3, 1e-3, device=0, incremental_update=True),
    lambda: abo.HipShardedGP(abo.Matern52Kernel(), 1e-3, devices=[0, 0], incremental_update=True),
    lambda: abo.HipShardedGradientGP(abo.Matern52Kernel(), 3, 1e-3, devices=[0, 0], incremental_update=True),
])
def test_flag_survives_the_driver_rebuilds(make):
    m = make()
    assert m.incremental_update is True
    assert abo.copy(m).incremental_update is True
    assert type(abo.copy(m)) is type(m)
    sigma = np.array([2.0, 2.0, 2.0]) if hasattr(m, "p") else 2.0
    assert abo.rescale_model(m, sigma).incremental_update is True
    assert abo._update_model_parameters(m, 1.5 * abo.with_lengthscale(abo.Matern52Kernel(), 0.7)).incremental_update is True
    if not hasattr(m, "devices"):                              # a sharded group is not picklable (rebuilt from its data)
        assert pickle.loads(pickle.dumps(m)).incremental_update is True
    # and it stays off unless asked for
    off = type(m).__new__(type(m))
    assert getattr(off, "incremental_update", False) is False
    assert abo.HipStandardGP(abo.Matern52Kernel(), 1e-3, device=0).incremental_update is False


def test_julia_shims_bind_update_with_the_header_prototype():
    protos = c_prototypes()
    for path in SHIMS:
        calls = [c for c in julia_calls(path) if c[0] in NAMES]
        assert {c[0] for c in calls} == set(NAMES), path
        for name, types, ret, line in calls:
            want = protos[name]
            assert ret == "Int32" and len(types) == len(want), f"{path}:{line} {name}"
            for jl, c in zip(types, want):
                assert jl_matches_c(jl, c), f"{path}:{line} {name}: {jl} vs {c}"
        src = open(path).read()
        assert re.search(r"incremental_update\s*=\s*false", src), path
        assert "m.incremental" in src and "_with(" in src
