"""HipStandardGP — the MI355X-resident drop-in for the reference's ``StandardGP <: AbstractSurrogate``
(src/surrogates/StandardGP.jl).  Same names, argument meaning and error behaviour as the reference's
methods; every floating-point operation of update / posterior / NLML runs in libabo_hip.so through
the C-ABI of include/abo_hip.h.  There is no CPU fallback.

Value semantics follow the reference: ``update`` returns a *new* model (StandardGP.jl:82), ``copy``
returns a distinct object that shares the immutable device state (StandardGP.jl:26 deep-copies
α, C, x, δ — 512 MiB per BO step at N = 8192; here it is one reference-count increment).
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import _lib
from ._lib import AboParams, AboTimings, DEVICE, HOST
from .kernels import ConstMean, Kernel, ZeroMean, extract_scale_and_lengthscale, is_ard, with_lengthscale


class AbstractSurrogate:
    """src/abstract.jl:33."""


def _is_torch(x):
    return type(x).__module__.startswith("torch") and hasattr(x, "data_ptr")


def as_points(x, d_expected=None):
    """Accept the reference's input containers: a length-M vector of reals (d = 1,
    test/test_surrogates.jl:67), a vector of d-vectors (acq_utils.jl:47), an (M, d) array, or a
    contiguous float64 torch tensor (host or on the model's GPU).
    Returns (pointer, M, d, space, keepalive)."""
    if _is_torch(x):
        import torch
        t = x
        if t.dtype != torch.float64:
            raise TypeError("torch inputs must be float64")
        if t.dim() == 1:
            t = t[:, None]
        if t.dim() != 2:
            raise _lib.DimensionMismatch("inputs must be (M,) or (M, d)")
        t = t.contiguous()
        if t.is_cuda:
            torch.cuda.current_stream(t.device).synchronize()   # the library runs on its own stream
        return t.data_ptr(), t.shape[0], t.shape[1], (DEVICE if t.is_cuda else HOST), t
    try:
        a = np.asarray(x, dtype=np.float64)
    except ValueError as e:   # ragged vector-of-vectors
        raise _lib.DimensionMismatch(f"input points differ in length: {e}") from None
    if a.ndim == 1:
        a = a[:, None]
    if a.ndim != 2:
        raise _lib.DimensionMismatch("inputs must be (M,) or (M, d)")
    a = np.ascontiguousarray(a)
    return a.ctypes.data, a.shape[0], a.shape[1], HOST, a


class ArdUnsupported(TypeError):
    """an entry point that takes or returns coordinates and does not scale them was handed a model with per-coordinate length scales"""


def ard_lengthscales(model):
    """the d length scales of an ARD model as an array, None for a model with one scalar length scale"""
    ell = getattr(getattr(model, "kernel", None), "lengthscale", None)
    return np.asarray(ell, dtype=np.float64) if isinstance(ell, tuple) else None


def refuse_ard(model, what: str) -> None:
    """the one error of every entry point that would otherwise treat an ARD model as isotropic"""
    if ard_lengthscales(model) is not None:
        raise ArdUnsupported(f"{what} does not support ARD length scales (one per coordinate): its coordinates would cross the "
                             "library unscaled; use a scalar length scale, or pre-divide the coordinates yourself")


def _ard_scale(model, x, inverse: bool, bounds: bool):
    ell = ard_lengthscales(model)
    if ell is None or x is None:
        return x
    if np.isscalar(x):
        x = [float(x)]
    if not _is_torch(x):
        try:
            x = np.asarray(x, dtype=np.float64)
        except ValueError as e:   # ragged vector-of-vectors
            raise _lib.DimensionMismatch(f"input points differ in length: {e}") from None
    nd = x.dim() if _is_torch(x) else x.ndim
    # as_points' reading of the containers: a vector is M points of dimension 1 — unless it is a box bound or one point (bounds)
    vector_of_scalars = nd == 1 and not bounds
    d = 1 if vector_of_scalars else (x.shape[-1] if nd >= 1 else 0)
    if d != ell.shape[0]:
        raise _lib.DimensionMismatch(f"the model has {ell.shape[0]} length scales, the points have dimension {d}")
    if _is_torch(x):
        import torch
        e = torch.as_tensor(ell, dtype=x.dtype, device=x.device)       # d values; the points stay where they are
    else:
        e = ell
    if vector_of_scalars:
        e = e[0]
    return x * e if inverse else x / e


def to_model_space(model, x, bounds: bool = False):
    """Points in any container `as_points` reads — or, with bounds=True, a box bound / one point as a d-vector — → the coordinates the
    library sees.  An ARD model (a kernel with
    one length scale per coordinate) crosses the C-ABI as ell = 1 on coordinates divided by their ℓ_c (include/abo_hip.h:
    abo_nlml_grad_ard); any other model's points pass through untouched.  NumPy in, NumPy out; a torch tensor is scaled with torch on
    its own device."""
    return _ard_scale(model, x, False, bounds)


def from_model_space(model, x, bounds: bool = False):
    """the inverse of `to_model_space`: what the library returns as coordinates, multiplied back by ℓ_c"""
    return _ard_scale(model, x, True, bounds)


class _Handle:
    """Owns one abo_gp reference."""

    def __init__(self, ptr):
        self.ptr = ptr

    def __del__(self):
        try:
            if self.ptr:
                _lib.lib().abo_destroy(self.ptr)
                self.ptr = None
        except Exception:
            pass


class HipStandardGP(AbstractSurrogate):
    """StandardGP(kernel, noise_var; mean=nothing) (src/surrogates/StandardGP.jl:41-64)."""

    def __init__(self, kernel: Kernel, noise_var: float, mean=None, device: int | None = None, jitter: float = 0.0,
                 chunk: int = 0, n_max: int = 0, contraction: str | None = None, incremental_update: bool = False):
        if mean is None:
            mean = ZeroMean()
        inner, scale, ell = extract_scale_and_lengthscale(kernel)
        ell = 1.0 if ell is None else ell
        self.kernel = scale * with_lengthscale(inner, ell)     # normal form
        self.noise_var = noise_var
        self.mean = mean
        self.jitter = float(jitter)
        self.chunk = int(chunk)
        self.n_max = int(n_max)          # capacity for incremental appends (0 = size to the fit)
        # engine of the variance contraction: None = the library default (auto), "fp64", "int8" or "int8:<moduli>"
        self.contraction = contraction
        parse_contraction(contraction)
        # update(model, xs, ys) on a fitted model: bordered appends when (xs, ys) extends its data (abo_update), else the refit;
        # off = always the refit, the reference's arithmetic
        self.incremental_update = bool(incremental_update)
        self.update_path = None   # what the update that made this model ran: "shared" / "appended" / "refit"
        self._d = None            # input dimension of the data the model is conditioned on (set by update; None: ask the library)
        if device is None:
            device = _current_device()
        self.device = int(device)
        self._h = None            # gpx === nothing

    # -- reference field names -------------------------------------------------------------------
    @property
    def gpx(self):
        return self._h

    @property
    def gp(self):
        return (self.mean, self.kernel)

    def _params(self) -> AboParams:
        # ARD: the length scales live in the coordinates (to_model_space), the library sees ell = 1
        ell = 1.0 if is_ard(self.kernel) else float(self.kernel.lengthscale)
        return AboParams(family=self.kernel.family, device=self.device, ell=ell,
                         sigma_f2=float(self.kernel.scale), noise_var=float(self.noise_var),
                         mean_c=float(getattr(self.mean, "c", 0.0)), jitter=self.jitter, n_max=self.n_max, chunk=self.chunk)

    def _clone(self, handle):
        m = object.__new__(HipStandardGP)
        m.kernel, m.noise_var, m.mean, m.jitter, m.chunk, m.device, m.n_max = (self.kernel, self.noise_var, self.mean,
                                                                              self.jitter, self.chunk, self.device, self.n_max)
        m.contraction = getattr(self, "contraction", None)
        m.incremental_update = getattr(self, "incremental_update", False)
        m.update_path = getattr(self, "update_path", None)
        m._d = getattr(self, "_d", None)
        m._h = handle
        return m

    def _require(self):
        if self._h is None:
            raise ValueError("surrogate is not conditioned on data yet (gpx === nothing): call update first")
        return self._h.ptr

    def timings(self) -> dict:
        t = AboTimings()
        _lib.check(_lib.lib().abo_get_timings(self._require(), C.byref(t)))
        return t.as_dict()

    def prune_stats(self) -> dict:
        """the pruned top-k selection of the last evaluate() on this model (include/abo_hip.h: abo_prune_stats)"""
        t = _lib.AboPruneStats()
        _lib.check(_lib.lib().abo_get_prune_stats(self._require(), C.byref(t)))
        return t.as_dict()

    def prune_levels(self) -> dict:
        """the bound levels of the same call (include/abo_hip.h: abo_get_prune_levels): rows and survivors of the first level over all
        candidates and of the second over its survivors — rows 0: that level did not run —, and the ms each took"""
        o = (C.c_int64 * 6)()
        _lib.check(_lib.lib().abo_get_prune_levels(self._require(), o))
        return {"level1_rows": o[0], "level1_survivors": o[1], "level2_rows": o[2], "level2_survivors": o[3],
                "level1_ms": o[4] * 1e-3, "level2_ms": o[5] * 1e-3}

    # Checkpoint / resume: the reference has no serialisation code, a BOStruct is rebuilt from (xs, ys, hyper-
    # parameters) (bayesian_opt.jl:81).  A pickled model is exactly that — hyper-parameters plus the training data
    # read back from the device — and unpickling refits on the current device.
    def __getstate__(self):
        st = {k: v for k, v in self.__dict__.items() if k != "_h"}
        st["_data"] = training_data(self) if self._h is not None else None
        return st

    def __setstate__(self, st):
        data = st.pop("_data", None)
        self.__dict__.update(st)
        self._h = None
        self.device = _current_device()
        if data is not None:
            import abstractbayesopt.jl_amd as _pkg
            self._h = _pkg.update(self, data[0], data[1])._h

    def __copy__(self):
        return copy(self)

    def __repr__(self):
        return f"HipStandardGP({self.kernel!r}, noise_var={self.noise_var}, mean={self.mean}, fitted={self._h is not None})"


def parse_contraction(spec):
    """"auto" | "fp64" | "int8" | "int8:<moduli>" → (engine, moduli) of abo_set_contraction (include/abo_hip.h)."""
    if spec is None:
        return _lib.CONTRACT_AUTO, 0
    name, _, n = str(spec).partition(":")
    engines = {"auto": _lib.CONTRACT_AUTO, "fp64": _lib.CONTRACT_FP64, "int8": _lib.CONTRACT_INT8}
    if name not in engines or (n and not n.isdigit()):
        raise ValueError(f"contraction must be auto, fp64, int8 or int8:<moduli>, not {spec!r}")
    return engines[name], int(n) if n else 0


def set_default_contraction(spec) -> None:
    """Process-wide default engine of the variance contraction for handles created from now on."""
    _lib.check(_lib.lib().abo_set_contraction(None, *parse_contraction(spec)))


def _current_device() -> int:
    try:
        import torch
        if torch.cuda.is_available():
            return torch.cuda.current_device()
    except Exception:
        pass
    return 0


# ---- Base.copy ---------------------------------------------------------------------------------
def copy(model: HipStandardGP) -> HipStandardGP:
    """Base.copy(s::StandardGP) (StandardGP.jl:26): `copied.gp === orig.gp`, `copied.gpx !== orig.gpx`
    (test/test_surrogates.jl:139-142)."""
    if model._h is None:
        return model._clone(None)
    _lib.check(_lib.lib().abo_retain(model._h.ptr))
    return model._clone(_Handle(model._h.ptr))


# ---- update --------------------------------------------------------------------------------------
def update(model: HipStandardGP, xs, ys) -> HipStandardGP:
    """update(model::StandardGP, xs, ys) (StandardGP.jl:79-83): full refit, returns a new model.
    Raises PosDefException(info) when K + σ²I is not positive definite (no jitter unless the model
    was built with jitter > 0) and DimensionMismatch on ragged / mismatched inputs."""
    xs = to_model_space(model, xs)
    L = _lib.lib()
    xp, n, d, xspace, xkeep = as_points(xs)
    if _is_torch(ys):
        import torch
        yt = ys.reshape(-1).contiguous()
        if yt.dtype != torch.float64:
            raise TypeError("torch targets must be float64")
        yspace = DEVICE if yt.is_cuda else HOST
        yp, ny, ykeep = yt.data_ptr(), yt.shape[0], yt
    else:
        ya = np.ascontiguousarray(np.asarray(ys, dtype=np.float64).reshape(-1))
        yspace, yp, ny, ykeep = HOST, ya.ctypes.data, ya.shape[0], ya
    if ny != n:
        raise _lib.DimensionMismatch(f"xs has {n} points but ys has {ny} values")
    if xspace != yspace:
        raise ValueError("xs and ys must both be host arrays or both be tensors on the model's GPU")
    hp = C.c_void_p()
    prm = model._params()
    info = C.c_int64(0)
    if getattr(model, "incremental_update", False) and model._h is not None:
        path = C.c_int32(_lib.UPDATE_REFIT)
        st = L.abo_update(model._h.ptr, C.byref(prm), None, xp, n, d, yp, xspace, C.byref(info), C.byref(path), C.byref(hp))
        _lib.check(st, info.value)
        h = _Handle(hp.value)
        if getattr(model, "contraction", None) is not None:
            _lib.check(L.abo_set_contraction(h.ptr, *parse_contraction(model.contraction)))
        del xkeep, ykeep
        return _with_path(model._clone(h), path.value, d)
    _lib.check(L.abo_create(C.byref(prm), C.byref(hp)))
    h = _Handle(hp.value)
    if getattr(model, "contraction", None) is not None:
        _lib.check(L.abo_set_contraction(h.ptr, *parse_contraction(model.contraction)))
    st = L.abo_fit(h.ptr, xp, n, d, yp, xspace, C.byref(info))
    _lib.check(st, info.value)
    del xkeep, ykeep
    return _with_path(model._clone(h), _lib.UPDATE_REFIT, d)


def _with_path(model, path: int, d=None):
    model.update_path = _lib.UPDATE_PATHS[path]
    if d is not None:
        model._d = int(d)
    return model


# ---- posterior -----------------------------------------------------------------------------------
def _predict(model, x, want_mu, want_var):
    if np.isscalar(x):                       # abstract.jl:67-69 scalar wrapper
        x = [float(x)]
    x = to_model_space(model, x)
    L = _lib.lib()
    zp, m, d, zspace, keep = as_points(x)
    if hasattr(model, "devices") and zspace == HOST:          # HipShardedGP: shard the batch over the group's devices
        from . import multigpu
        mu, var = multigpu.mean_and_var(model, keep)
        return (mu if want_mu else None), (var if want_var else None)
    if zspace == DEVICE:
        import torch
        mu = torch.empty(m, dtype=torch.float64, device=keep.device) if want_mu else None
        var = torch.empty(m, dtype=torch.float64, device=keep.device) if want_var else None
        st = L.abo_predict(model._require(), zp, m, d, DEVICE, mu.data_ptr() if want_mu else None,
                           var.data_ptr() if want_var else None, DEVICE)
    else:
        mu = np.empty(m) if want_mu else None
        var = np.empty(m) if want_var else None
        st = L.abo_predict(model._require(), zp, m, d, HOST, mu.ctypes.data if want_mu else None,
                           var.ctypes.data if want_var else None, HOST)
    _lib.check(st)
    return mu, var


def posterior_mean(model: HipStandardGP, x):
    """posterior_mean (StandardGP.jl:329-331, :361-363): mean(model.gpx(x))."""
    return _predict(model, x, True, False)[0]


def posterior_var(model: HipStandardGP, x):
    """posterior_var (StandardGP.jl:345-347, :377-379): var(model.gpx(x)) — latent variance + 1e-18."""
    return _predict(model, x, False, True)[1]


def mean_and_var(model: HipStandardGP, x):
    """[upstream AbstractGPs] mean_and_var(model.gpx(x)) — one fused pass (StandardGP.jl:399)."""
    return _predict(model, x, True, True)


def unstandardized_mean_and_var(model: HipStandardGP, xs, params):
    """unstandardized_mean_and_var (StandardGP.jl:395-404)."""
    mu, sigma = params
    m, v = mean_and_var(model, xs)
    return m * sigma + mu, v * sigma ** 2


# ---- joint posterior covariance (abo_predict_cov) ------------------------------------------------------
COV_MAX_POINTS = 8192


def _cov_model(model, what: str):
    """the models abo_predict_cov serves: a single-device HipStandardGP — refused on the host, before anything is staged"""
    if hasattr(model, "devices"):
        raise TypeError(f"{what}: a sharded model (HipShardedGP) is not supported: the factor is spread over its devices; "
                        "use a single-device HipStandardGP")
    if hasattr(model, "p"):
        raise TypeError(f"{what}: a gradient-enhanced model (HipGradientGP) has p outputs per point; posterior_grad_cov gives the "
                        "p × p block of one point")
    if not isinstance(model, HipStandardGP):
        raise TypeError(f"{what} needs a HipStandardGP, not {type(model).__name__}")


def _cov_points(model, x, name: str):
    if np.isscalar(x):
        x = [float(x)]
    p, m, d, space, keep = as_points(to_model_space(model, x))
    want = getattr(model, "_d", None)
    if want is not None and d != want:
        raise _lib.DimensionMismatch(f"DimensionMismatch: {name} has dimension {d}, model dimension {want}")
    if not 1 <= m <= COV_MAX_POINTS:
        raise ValueError(f"{name} holds {m} points; abo_predict_cov takes 1 to {COV_MAX_POINTS} per set")
    return p, m, d, space, keep


def _predict_cov(model, xa, xb, want_mu: bool, what: str):
    """(mu_a, cov) through one abo_predict_cov; xb None: the symmetric form.  Host inputs give NumPy arrays, tensors on the model's GPU
    give tensors there."""
    _cov_model(model, what)
    pa, ma, d, space, keep_a = _cov_points(model, xa, "xa")
    pb, mb, keep_b = None, ma, None
    if xb is not None:
        pb, mb, db, space_b, keep_b = _cov_points(model, xb, "xb")
        if db != d:
            raise _lib.DimensionMismatch(f"DimensionMismatch: xa has dimension {d}, xb has dimension {db}")
        if space_b != space:
            raise ValueError("xa and xb must both be host arrays or both be tensors on the model's GPU")
    h = model._require()
    if space == DEVICE:
        import torch
        cov = torch.empty((ma, mb), dtype=torch.float64, device=keep_a.device)
        mu = torch.empty(ma, dtype=torch.float64, device=keep_a.device) if want_mu else None
        st = _lib.lib().abo_predict_cov(h, pa, ma, pb, mb if xb is not None else 0, d, DEVICE, mu.data_ptr() if want_mu else None, None,
                                        cov.data_ptr(), DEVICE)
    else:
        cov = np.empty((ma, mb), dtype=np.float64)
        mu = np.empty(ma, dtype=np.float64) if want_mu else None
        st = _lib.lib().abo_predict_cov(h, pa, ma, pb, mb if xb is not None else 0, d, HOST, mu.ctypes.data if want_mu else None, None,
                                        cov.ctypes.data, HOST)
    _lib.check(st)
    del keep_a, keep_b
    return mu, cov


def posterior_cov(model: HipStandardGP, xa, xb=None):
    """[upstream AbstractGPs] cov(model.gpx(xa)) and cov(model.gpx(xa), model.gpx(xb)): the (Ma, Mb) joint latent posterior covariance
    (no observation noise).  xb None: the symmetric form — symmetric bit for bit, its diagonal posterior_var's (with the 1e-18).
    1 to 8192 points per set.  An ARD model is served through `to_model_space`; a covariance needs no back-scaling."""
    return _predict_cov(model, xa, xb, False, "posterior_cov")[1]


def mean_and_cov(model: HipStandardGP, x):
    """[upstream AbstractGPs] mean_and_cov(model.gpx(x)) → (mu, cov) from one call."""
    return _predict_cov(model, x, None, True, "mean_and_cov")


def sample_joint(model: HipStandardGP, x, n: int, rng=None, jitter=None):
    """[upstream AbstractGPs] rand(model.gpx(x), n), transposed: (n, M) exact draws of the latent posterior at the M points x —
    mu + L·ξ with L the host Cholesky factor of cov + jitter·I (an M × M factorisation: host work by design).  jitter None: the ladder
    1e-12·σ_f² … 1e-6·σ_f², × 10 per failed factorisation, then PosDefException; a number: that jitter alone.  rng: a
    numpy.random.Generator (or a seed)."""
    n = int(n)
    if n < 0:
        raise ValueError("sample_joint: n must be non-negative")
    mu, cov = mean_and_cov(model, x)
    if _is_torch(cov):
        mu, cov = mu.cpu().numpy(), cov.cpu().numpy()
    sf2 = float(model.kernel.scale)
    ladder = [float(jitter)] if jitter is not None else [sf2 * 10.0 ** e for e in range(-12, -5)]
    m = cov.shape[0]
    for j in ladder:
        try:
            chol = np.linalg.cholesky(cov + j * np.eye(m))
        except np.linalg.LinAlgError:
            continue
        if not np.all(np.isfinite(chol)):
            continue
        rng = rng if isinstance(rng, np.random.Generator) else np.random.default_rng(rng)
        return mu[None, :] + rng.standard_normal((n, m)) @ chol.T
    raise _lib.PosDefException(0, f"sample_joint: the {m} × {m} posterior covariance is not positive definite with a jitter of up to "
                                  f"{ladder[-1]:.3e}")


# ---- knowledge gradient over a discrete decision set (abo_acq_kg) -----------------------------------------
KG_CHUNK = COV_MAX_POINTS          # candidates per abo_acq_kg call


def _host_top_k(scores, k):
    """the library's order on the host: descending, ties to the lowest index, NaN first; (NaN, −1) behind len(scores) < k"""
    s = np.asarray(scores, dtype=np.float64)
    key = np.where(np.isnan(s), np.inf, s)
    order = np.argsort(-key, kind="stable")[:k]
    val, idx = np.full(k, np.nan), np.full(k, -1, dtype=np.int64)
    val[:order.shape[0]], idx[:order.shape[0]] = s[order], order
    return val, idx


def knowledge_gradient(model: HipStandardGP, candidates, decision=None, noise=None, include_self=True, k: int = 0):
    """Knowledge gradient of every candidate over a discrete decision set (minimisation): the expected decrease of
    min_j μ(decision_j) from one observation at the candidate (Frazier, Powell and Dayanik 2009; include/abo_hip.h: abo_acq_kg).
    decision None: the candidates themselves (the symmetric form; include_self is ignored); else up to 8192 points, and include_self
    adds each candidate's own point to its row (KGCP — what one wants when `decision` is the training set).  noise None: the noise the
    factor was built with; a number ≥ 0: that observation noise.  Returns the scores, and (scores, top_val, top_idx) when k > 0 —
    descending, ties to the lowest index.  Host inputs give NumPy arrays, tensors on the model's GPU give tensors there.  More than
    8192 candidates against a given decision set run in chunks of 8192, their selections merged on the host in the same order; the
    symmetric form takes at most 8192.  An ARD model is served through `to_model_space`."""
    what = "knowledge_gradient"
    _cov_model(model, what)
    k = int(k)
    if k < 0:
        raise ValueError(f"{what}: k = {k} is negative")
    nz = -1.0 if noise is None else float(noise)
    if noise is not None and not (math.isfinite(nz) and nz >= 0.0):
        raise ValueError(f"{what}: noise must be a finite number ≥ 0 (None: the model's own), got {noise}")
    if np.isscalar(candidates):
        candidates = [float(candidates)]
    pa, ma, d, space, keep_a = as_points(to_model_space(model, candidates))
    want = getattr(model, "_d", None)
    if want is not None and d != want:
        raise _lib.DimensionMismatch(f"DimensionMismatch: candidates have dimension {d}, model dimension {want}")
    if ma < 1:
        raise ValueError(f"{what}: no candidates")
    pb, mb, keep_b, flags = None, 0, None, 0
    if decision is None:
        if ma > COV_MAX_POINTS:
            raise ValueError(f"{what}: the symmetric form (decision=None) takes 1 to {COV_MAX_POINTS} candidates, got {ma}")
    else:
        pb, mb, db, space_b, keep_b = _cov_points(model, decision, "decision")
        if db != d:
            raise _lib.DimensionMismatch(f"DimensionMismatch: candidates have dimension {d}, decision has dimension {db}")
        if space_b != space:
            raise ValueError("candidates and decision must both be host arrays or both be tensors on the model's GPU")
        flags = _lib.KG_SELF if include_self else 0
    h = model._require()
    on_device = space == DEVICE
    if on_device:
        import torch
        scores = torch.empty(ma, dtype=torch.float64, device=keep_a.device)
    else:
        scores = np.empty(ma, dtype=np.float64)
    chunk = max(1, int(KG_CHUNK))
    nchunks = (ma + chunk - 1) // chunk
    parts = []
    for c in range(nchunks):
        i0 = c * chunk
        n = min(chunk, ma - i0)
        kk = min(k, n) if nchunks > 1 else k          # (a chunk's selection never needs more than its own points)
        if on_device:
            tv = torch.empty(kk, dtype=torch.float64, device=keep_a.device)
            ti = torch.empty(kk, dtype=torch.int64, device=keep_a.device)
            ptrs = (scores[i0:].data_ptr(), tv.data_ptr() if kk else None, ti.data_ptr() if kk else None)
        else:
            tv, ti = np.empty(kk, dtype=np.float64), np.empty(kk, dtype=np.int64)
            ptrs = (scores[i0:].ctypes.data, tv.ctypes.data if kk else None, ti.ctypes.data if kk else None)
        st = _lib.lib().abo_acq_kg(h, pa + i0 * d * 8, n, pb, mb, d, space, nz, flags, i0, ptrs[0], kk, ptrs[1], ptrs[2], space)
        _lib.check(st)
        parts.append((tv, ti))
    del keep_b
    if k == 0:
        return scores
    if nchunks == 1:
        return scores, parts[0][0], parts[0][1]
    # merge on the host: the chunks' selections hold every candidate of the overall selection; ranked by (score, index) in the library's order
    if on_device:
        cv = np.concatenate([p[0].cpu().numpy() for p in parts])
        ci = np.concatenate([p[1].cpu().numpy() for p in parts])
    else:
        cv, ci = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
    by_index = np.argsort(ci, kind="stable")                       # ties to the lowest candidate index
    val, pos = _host_top_k(cv[by_index], k)
    idx = np.where(pos >= 0, ci[by_index][np.maximum(pos, 0)], -1)
    if on_device:
        import torch
        return scores, torch.from_numpy(val).to(keep_a.device), torch.from_numpy(idx).to(keep_a.device)
    return scores, val, idx


# ---- NLML ----------------------------------------------------------------------------------------
def nlml_fitted(model: HipStandardGP) -> float:
    """NLML of the model's own fitted state (no refit)."""
    out = C.c_double()
    _lib.check(_lib.lib().abo_nlml(model._require(), C.byref(out)))
    return out.value


def nlml(model: HipStandardGP, params, xs, ys) -> float:
    """nlml(model, params, xs, ys) (StandardGP.jl:99-114): params = [log ℓ, log scale]; rebuilds the
    kernel with exp.(params), keeps noise and mean, returns −logpdf (value only — ForwardDiff duals
    cannot cross a C-ABI; SURVEY.md §8(f) rank 2 tracks the analytic gradient)."""
    if len(params) > 2:
        # ARD: params = [log ℓ_1 … log ℓ_d, log scale] (hyperparams.nlml_and_grad_ard is the same with the gradient; at d = 1 the two
        # parameter sets coincide)
        k = math.exp(params[-1]) * with_lengthscale(get_kernel_constructor(model), [math.exp(p) for p in params[:-1]])
        g = HipStandardGP(k, model.noise_var, mean=model.mean, device=model.device, jitter=model.jitter, contraction=model.contraction)
        return nlml_fitted(update(g, xs, ys))
    log_ell, log_scale = params
    if hasattr(log_ell, "partials") or hasattr(log_scale, "partials"):
        # dual-number parameters (what Optim's autodiff=:forward feeds the objective, bayesian_opt.jl:276-285): value and
        # analytic gradient at the values, partials through the chain rule
        from .hyperparams import nlml_dual
        return nlml_dual(model, (log_ell, log_scale), xs, ys)
    k = math.exp(log_scale) * with_lengthscale(get_kernel_constructor(model), math.exp(log_ell))
    g = HipStandardGP(k, model.noise_var, mean=model.mean, device=model.device, jitter=model.jitter, contraction=model.contraction)
    return nlml_fitted(update(g, xs, ys))


def leave_one_out(model: HipStandardGP):
    """(mu, var, lpd, nlpl): the leave-one-out predictive mean and variance of every observed target (noise included), its log
    predictive density under them, and nlpl = −Σ lpd — from the fitted model's resident L⁻¹ in one pass (abo_loo; no refit).
    NumPy arrays of the model's N.  An ARD model is served as it is: no coordinates cross the call."""
    h = model._require()
    n, d = C.c_int64(), C.c_int32()
    _lib.check(_lib.lib().abo_get_n(h, C.byref(n), C.byref(d)))
    mu, var, lpd = (np.empty(n.value, dtype=np.float64) for _ in range(3))
    v = C.c_double()
    _lib.check(_lib.lib().abo_loo(h, mu.ctypes.data, var.ctypes.data, lpd.ctypes.data, C.byref(v), HOST))
    return mu, var, lpd, v.value


def nlml_ls(model: HipStandardGP, log_ell, log_scale, xs, ys) -> float:
    """nlml_ls (StandardGP.jl:133-149)."""
    return nlml(model, (log_ell, log_scale), xs, ys)


# ---- standardisation helpers (host-side scalars; StandardGP.jl:164-232) -----------------------------
def get_mean_std(model: HipStandardGP, y_train, choice: str):
    y = np.asarray(y_train, dtype=np.float64).reshape(-1)
    y_mean, y_std = float(np.mean(y)), float(np.std(y, ddof=1))
    if choice == "scale_only":
        y_mean = 0.0
    elif choice == "mean_only":
        y_std = 1.0
    return y_mean, y_std


def std_y(model: HipStandardGP, ys, mu, sigma):
    return (np.asarray(ys, dtype=np.float64) - mu) / sigma


def rescale_model(model: HipStandardGP, sigma):
    ell = model.kernel.lengthscale
    new_scale = get_scale(model)[0] / sigma ** 2
    new_kernel = new_scale * with_lengthscale(get_kernel_constructor(model), ell)
    mean = model.mean
    if not isinstance(mean, ZeroMean):
        mean = ConstMean(mean.c / sigma)
    return HipStandardGP(new_kernel, model.noise_var / sigma ** 2, mean=mean, device=model.device,
                         jitter=model.jitter, chunk=model.chunk, n_max=model.n_max, contraction=model.contraction,
                         incremental_update=getattr(model, "incremental_update", False))


def _update_model_parameters(model: HipStandardGP, kernel: Kernel):
    return HipStandardGP(kernel, model.noise_var, mean=model.mean, device=model.device, jitter=model.jitter,
                         chunk=model.chunk, n_max=model.n_max, contraction=model.contraction,
                         incremental_update=getattr(model, "incremental_update", False))


def get_lengthscale(model: HipStandardGP):
    """1-element vector, as the reference returns (StandardGP.jl:261; test_surrogates.jl:32-33); the d values of an ARD model."""
    ell = model.kernel.lengthscale
    return list(ell) if isinstance(ell, tuple) else [ell]


def get_scale(model: HipStandardGP):
    return [model.kernel.scale]


def get_kernel_constructor(model: HipStandardGP) -> Kernel:
    return Kernel(model.kernel.family)


def prep_input(model: HipStandardGP, xs):
    return xs


def prep_output(model: HipStandardGP, ys):
    return ys


def _get_minimum(model: HipStandardGP, ys):
    """_get_minimum (StandardGP.jl:418)."""
    return float(np.min(np.asarray(ys, dtype=np.float64)))


def get_factor(model: HipStandardGP):
    """(L, alpha, Linv) of the fitted state as host arrays — test introspection."""
    n = C.c_int64()
    d = C.c_int32()
    Lb = _lib.lib()
    _lib.check(Lb.abo_get_n(model._require(), C.byref(n), C.byref(d)))
    N = n.value * getattr(model, "p", 1)          # factor rows: p outputs per point for a gradient-enhanced model
    Lm, Li, al = np.empty((N, N)), np.empty((N, N)), np.empty(N)
    _lib.check(Lb.abo_get_factor(model._require(), Lm.ctypes.data, al.ctypes.data, Li.ctypes.data))
    return Lm, al, Li


def training_data(model: HipStandardGP):
    """(X, y) the model is conditioned on, read back from the device: X (N, d) and y (N,) — for a gradient-enhanced
    model y is (N, p), one row [f, ∇f] per point, the shape `update` takes."""
    n = C.c_int64()
    d = C.c_int32()
    Lb = _lib.lib()
    _lib.check(Lb.abo_get_n(model._require(), C.byref(n), C.byref(d)))
    p = getattr(model, "p", 1)
    X, y = np.empty((n.value, d.value)), np.empty(n.value * p)
    _lib.check(Lb.abo_get_data(model._require(), X.ctypes.data, y.ctypes.data))
    return from_model_space(model, X), (y if p == 1 else np.ascontiguousarray(y.reshape(p, n.value).T))
