"""Thompson sampling: pathwise posterior sample paths (include/abo_hip.h: abo_paths_*).  No reference counterpart — the
reference's acquisitions are EI, UCB, PI, GradientNormUCB and ensembles of them.

A posterior sample is g_s(z) = f_s(z) + k(z, X)·v_s with a prior draw f_s in R random Fourier features and the exact kernel row
(Matheron's rule; Wilson et al. 2020).  The base randomness (frequencies, phases, feature weights, noise draws) is drawn HERE, on the
host, and handed to the library: the paths are a deterministic function of it, and a `SamplePaths` keeps the four arrays so that
anyone can restate its values.  The reference minimises, so a Thompson pick is the arg-min of a path."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import DEVICE, HOST
from .kernels import MATERN32, MATERN52, MATERN72, SE
from .surrogate import HipStandardGP, _is_torch, as_points, refuse_ard

_NU = {MATERN32: 1.5, MATERN52: 2.5, MATERN72: 3.5}


def _rng(rng):
    return rng if isinstance(rng, np.random.Generator) else np.random.default_rng(rng)


def spectral_frequencies(kernel, R: int, d: int, rng=None) -> np.ndarray:
    """R frequencies (R × d) of the UNIT-lengthscale kernel of `kernel`'s family, i.e. draws from its spectral density:
    SE → N(0, I); Matérn-ν (ν = 3/2, 5/2, 7/2) → N(0, I) / sqrt(χ²_{2ν} / 2ν), the multivariate Student-t with 2ν degrees of
    freedom.  With phases uniform in [0, 2π), E[2·cos(ω·x + b)·cos(ω·z + b)] = κ(‖x − z‖)."""
    family = getattr(kernel, "family", kernel)
    rng = _rng(rng)
    R, d = int(R), int(d)
    if R < 1 or d < 1:
        raise ValueError(f"spectral_frequencies: R = {R}, d = {d}")
    z = rng.standard_normal((R, d))
    if family == SE:
        return z
    if family not in _NU:
        raise ValueError(f"spectral_frequencies: unknown kernel family {family!r}")
    dof = 2.0 * _NU[family]
    return z / np.sqrt(rng.chisquare(dof, size=(R, 1)) / dof)


class _PathsHandle:
    def __init__(self, ptr):
        self.ptr = ptr

    def __del__(self):
        try:
            if self.ptr:
                _lib.lib().abo_paths_destroy(self.ptr)
                self.ptr = None
        except Exception:
            pass


def _is_resident(x):
    from .incremental import ResidentCandidates
    return isinstance(x, ResidentCandidates)


class SamplePaths:
    """S sample paths of one conditioned model.  Attributes omega (R × d), phase (R), w (S × R), eps (S × N): the base draws."""

    def __init__(self, model, omega, phase, w, eps):
        refuse_ard(model, "SamplePaths")
        if hasattr(model, "devices"):
            raise TypeError("sample paths of a sharded model (HipShardedGP) are not implemented: draw them from a single-device "
                            "HipStandardGP conditioned on the same data")
        if not isinstance(model, HipStandardGP):
            raise TypeError(f"sample paths need a HipStandardGP, not {type(model).__name__}")
        self.omega = np.ascontiguousarray(omega, dtype=np.float64)
        self.phase = np.ascontiguousarray(phase, dtype=np.float64)
        self.w = np.ascontiguousarray(w, dtype=np.float64)
        self.eps = np.ascontiguousarray(eps, dtype=np.float64)
        if self.w.ndim != 2:
            raise ValueError(f"SamplePaths: w must be (S, R), not {self.w.shape}")
        self.S, self.R = self.w.shape
        N, d = _model_shape(model)                      # (raises when the model is not conditioned on data)
        for name, a, want in (("omega", self.omega, (self.R, d)), ("phase", self.phase, (self.R,)), ("eps", self.eps, (self.S, N))):
            if a.shape != want:
                raise ValueError(f"SamplePaths: {name} has shape {a.shape}, the model (N = {N}, d = {d}) and w {self.w.shape} need {want}")
        self.model = model
        hp = C.c_void_p()
        _lib.check(_lib.lib().abo_paths_create(model._require(), self.S, self.R, self.omega.ctypes.data, self.phase.ctypes.data,
                                               self.w.ctypes.data, self.eps.ctypes.data, HOST, C.byref(hp)))
        self._h = _PathsHandle(hp.value)
        self._set = None

    def _eval(self, Z, want_values, k, idx_base=0):
        L, S, k = _lib.lib(), self.S, int(k)
        if _is_resident(Z):
            m, space, dev = Z.M, HOST, None
        else:
            zp, m, d, space, keep = as_points(Z)
            dev = keep.device if space == DEVICE else None
        if space == DEVICE:
            import torch
            values = torch.empty((S, m), dtype=torch.float64, device=dev) if want_values else None
            tv = torch.empty((S, k), dtype=torch.float64, device=dev) if k else None
            ti = torch.empty((S, k), dtype=torch.int64, device=dev) if k else None
            ptr = lambda a: a.data_ptr() if a is not None else None
        else:
            values = np.empty((S, m)) if want_values else None
            tv = np.empty((S, k)) if k else None
            ti = np.empty((S, k), dtype=np.int64) if k else None
            ptr = lambda a: a.ctypes.data if a is not None else None
        if _is_resident(Z):
            st = L.abo_paths_eval_cand(self._h.ptr, Z._h.ptr, int(idx_base), ptr(values), k, ptr(tv), ptr(ti), HOST)
        else:
            st = L.abo_paths_eval(self._h.ptr, zp, m, d, space, int(idx_base), ptr(values), k, ptr(tv), ptr(ti), space)
        _lib.check(st)
        return values, tv, ti

    def __call__(self, Z):
        """g_s(z_j) as an (S, M) array (NumPy for host inputs and resident sets, a torch tensor on the GPU for device inputs)"""
        return self._eval(Z, True, 0)[0]

    def argmin(self, Z, k: int = 1, idx_base: int = 0):
        """per path the k candidates with the smallest g_s: (values (S, k), indices (S, k)) in abo_acq's order on −g_s"""
        if k < 1:
            raise ValueError(f"argmin: k = {k}")
        _, tv, ti = self._eval(Z, False, k, idx_base)
        return tv, ti

    def stats(self) -> dict:
        st = _lib.AboPathsStats()
        _lib.check(_lib.lib().abo_paths_stats_get(self._h.ptr, C.byref(st)))
        return st.as_dict()

    # ---- following the model through appends (include/abo_hip.h: abo_paths_append …) ----
    def append(self, model2, eps_new=None, rng=None):
        """Advance the paths IN PLACE to `model2`, the one-point append of the model they describe (incremental.append): one fresh
        N(0,1) draw per path (`eps_new`, S values; drawn from `rng` when not given) joins `eps` as its last column, so that
        SamplePaths(model2, omega, phase, w, eps) restates the advanced paths.  With a set attached, the set must have been
        down-dated to `model2` first.  The advanced paths share their prior draw with the paths before: successive steps' paths are not
        independent draws.  Returns self."""
        if hasattr(model2, "devices") or not isinstance(model2, HipStandardGP):
            raise TypeError(f"SamplePaths.append needs the appended HipStandardGP, not {type(model2).__name__}")
        if eps_new is None:
            eps_new = _rng(rng).standard_normal(self.S)
        e = np.ascontiguousarray(eps_new, dtype=np.float64).reshape(-1)
        if e.shape != (self.S,):
            raise ValueError(f"SamplePaths.append: eps_new holds {e.shape[0]} values, the object has S = {self.S} paths")
        if not np.all(np.isfinite(e)):
            raise ValueError("SamplePaths.append: eps_new is not finite")
        _lib.check(_lib.lib().abo_paths_append(self._h.ptr, model2._require(), e.ctypes.data, HOST))
        self.eps = np.ascontiguousarray(np.concatenate([self.eps, e[:, None]], axis=1))     # (only after the library accepted the step)
        self.model = model2
        return self

    def attach(self, cand_set):
        """keep g_s(z_j) of every candidate of a ResidentCandidates set on the device (S × M doubles); the caller keeps the set alive
        while it is attached (the object holds a Python reference as well).  One set per object."""
        if not _is_resident(cand_set):
            raise TypeError(f"SamplePaths.attach needs a ResidentCandidates set, not {type(cand_set).__name__}")
        if getattr(self, "_set", None) is not None:
            raise ValueError("SamplePaths.attach: a set is attached already (detach() first)")
        _lib.check(_lib.lib().abo_paths_attach(self._h.ptr, cand_set._h.ptr))
        self._set = cand_set
        return self

    def detach(self):
        _lib.check(_lib.lib().abo_paths_detach(self._h.ptr))
        self._set = None

    def _attached(self, what):
        cs = getattr(self, "_set", None)
        if cs is None:
            raise ValueError(f"SamplePaths.{what}: no candidate set is attached (attach() first)")
        return cs

    def top(self, k: int = 1, idx_base: int = 0):
        """per path the k attached candidates with the smallest resident g_s: (values (S, k), indices (S, k)); k = 1 costs no pass"""
        k = int(k)
        if k < 1:
            raise ValueError(f"top: k = {k}")
        self._attached("top")
        tv, ti = np.empty((self.S, k)), np.empty((self.S, k), dtype=np.int64)
        _lib.check(_lib.lib().abo_paths_top(self._h.ptr, int(idx_base), k, tv.ctypes.data, ti.ctypes.data, HOST))
        return tv, ti

    def values(self) -> np.ndarray:
        """the resident values (S, M); +Inf at excluded candidates"""
        cs = self._attached("values")
        out = np.empty((self.S, cs.M))
        _lib.check(_lib.lib().abo_paths_values(self._h.ptr, out.ctypes.data, HOST))
        return out

    def append_stats(self) -> dict:
        st = _lib.AboPathsAppendStats()
        _lib.check(_lib.lib().abo_paths_append_stats_get(self._h.ptr, C.byref(st)))
        return st.as_dict()


def draw_base(kernel, S: int, R: int, N: int, d: int, rng=None):
    """the four base arrays of S paths in R features for a model of N points in d dimensions: (omega, phase, w, eps)"""
    rng = _rng(rng)
    omega = spectral_frequencies(kernel, R, d, rng)
    phase = rng.uniform(0.0, 2.0 * np.pi, size=R)
    w = rng.standard_normal((S, R))
    eps = rng.standard_normal((S, N))
    return omega, phase, w, eps


def _model_shape(model):
    n, d = C.c_int64(), C.c_int32()
    _lib.check(_lib.lib().abo_get_n(model._require(), C.byref(n), C.byref(d)))
    return n.value, d.value


def sample_paths(model, S: int, R: int = 1024, rng=None) -> SamplePaths:
    """S posterior sample paths of `model` in R random Fourier features; the base draws come from `rng` (a seed or a Generator)"""
    refuse_ard(model, "sample_paths")
    if hasattr(model, "devices"):
        raise TypeError("sample_paths: a sharded model (HipShardedGP) is not supported: draw the paths from a single-device "
                        "HipStandardGP conditioned on the same data")
    if not isinstance(model, HipStandardGP):
        raise TypeError(f"sample_paths needs a HipStandardGP, not {type(model).__name__}")
    N, d = _model_shape(model)
    return SamplePaths(model, *draw_base(model.kernel, int(S), int(R), N, d, rng))


def max_value_samples(model, Z, S: int, R: int = 1024, rng=None) -> np.ndarray:
    """S samples of the objective's minimum value for `acquisition.MaxValueEntropySearch`: the minimum of each of S posterior sample
    paths over the candidates Z (points, or a ResidentCandidates set) — `sample_paths(model, S, R, rng).argmin(Z, k=1)`'s values, bit for
    bit, as a host array (S,).  The minimum over a finite grid is an upper estimate of the path's true minimum."""
    S = int(S)
    if not 1 <= S <= 1024:
        raise ValueError(f"max_value_samples: S = {S} outside 1..1024 (the limit of MaxValueEntropySearch)")
    tv, _ = sample_paths(model, S, R, rng).argmin(Z, k=1)
    if _is_torch(tv):
        tv = tv.cpu().numpy()
    return np.ascontiguousarray(np.asarray(tv, dtype=np.float64)[:, 0])


def thompson_step(paths: SamplePaths, model2, cand_set, eps_new=None, rng=None, idx_base: int = 0):
    """One incremental Thompson step after `model2 = append(model, x, y)`: down-date the resident set to model2 (unless it is there
    already), advance the paths and their resident values, and return each path's arg-min (values (S,), indices (S,)).  The set is
    attached on first use."""
    if getattr(paths, "_set", None) is None:
        paths.attach(cand_set)
    elif paths._set is not cand_set:
        raise ValueError("thompson_step: the paths are attached to another candidate set")
    if cand_set.model is not model2:
        cand_set.downdate(model2)
    paths.append(model2, eps_new, rng)
    tv, ti = paths.top(1, idx_base)
    return tv[:, 0], ti[:, 0]


def distinct_picks(top_idx) -> np.ndarray:
    """path s takes its best index not taken by paths 0 … s − 1; top_idx: (q, k ≥ q) per-path orderings (−1: no candidate)"""
    taken, picks = set(), []
    for row in np.asarray(top_idx):
        for j in row:
            j = int(j)
            if j >= 0 and j not in taken:
                taken.add(j)
                picks.append(j)
                break
        else:
            raise ValueError(f"thompson_batch: path {len(picks)} has no candidate left that earlier paths did not take")
    return np.asarray(picks, dtype=np.int64)


def thompson_batch(model, Z, q: int, R: int = 1024, rng=None) -> np.ndarray:
    """q DISTINCT candidate indices (into Z, or into a ResidentCandidates set): the arg-mins of q independent sample paths, path s
    taking its best candidate not taken by paths 0 … s − 1"""
    q = int(q)
    if q < 1:
        raise ValueError(f"thompson_batch: q = {q}")
    paths = sample_paths(model, q, R, rng)
    _, ti = paths.argmin(Z, k=q)
    if _is_torch(ti):
        ti = ti.cpu().numpy()
    return distinct_picks(ti)
