"""NumPy restatement of the blocked bordered append (include/abo_hip.h: abo_append_batch; csrc/append_batch.hip): a factor state
(L, W = L⁻¹, α, log det, δᵀα) of N points conditioned on k more in one step, and the one-row bordered step abo_append takes, for
comparison.  Dense fp64, no GPU."""
import numpy as np


def refit(Kt, delta):
    """(L, W, α, log det K̃, δᵀα) of a dense refit"""
    L = np.linalg.cholesky(Kt)
    W = np.linalg.inv(L)
    alpha = W.T @ (W @ delta)
    return L, np.tril(W), alpha, 2.0 * np.sum(np.log(np.diag(L))), float(delta @ alpha)


def append_batch(L, W, alpha, logdet, quad, Kb, Kbb, delta_b):
    """One blocked step.  Kb = K̃[:N, N:] (N × k), Kbb = K̃[N:, N:] (k × k, noise on its diagonal), delta_b the k centred targets.
    Returns the new (L, W, α, log det, δᵀα).  Raises numpy.linalg.LinAlgError when S is not positive definite: with j = pivot_of(S),
    a refit's potrf reports that as N + j + 1."""
    N, k = Kb.shape
    B = np.tril(W) @ Kb                                  # pass 1: lower triangle of W
    S = Kbb - B.T @ B
    Ls = np.linalg.cholesky(S)
    Lsi = np.tril(np.linalg.inv(Ls))
    Cm = np.triu(W.T) @ B                                # pass 2: upper triangle of the stored Wᵀ
    r = delta_b - Kb.T @ alpha
    u = Lsi @ r
    beta = Lsi.T @ u
    Ln = np.zeros((N + k, N + k)); Wn = np.zeros((N + k, N + k))
    Ln[:N, :N] = L; Ln[N:, :N] = B.T; Ln[N:, N:] = Ls
    Wn[:N, :N] = W; Wn[N:, :N] = -Lsi @ Cm.T; Wn[N:, N:] = Lsi
    an = np.concatenate([alpha - Cm @ beta, beta])
    return Ln, Wn, an, logdet + 2.0 * np.sum(np.log(np.diag(Ls))), quad + float(u @ u)


def pivot_of(S):
    """0-based index of the first non-positive pivot of the Cholesky of S, or −1"""
    A = np.array(S, dtype=np.float64)
    for j in range(A.shape[0]):
        p = A[j, j] - A[j, :j] @ A[j, :j]
        if not p > 0.0:
            return j
        A[j, j] = np.sqrt(p)
        A[j + 1:, j] = (A[j + 1:, j] - A[j + 1:, :j] @ A[j, :j]) / A[j, j]
    return -1


def append_one(L, W, alpha, logdet, quad, kcol, kss, delta_new):
    """abo_append's bordered step (api.hip: append_impl): l = W·k, s² = k** + noise − ‖l‖², v = Wᵀ·l, β = (δ* − kᵀα)/s²"""
    N = L.shape[0]
    l = np.tril(W) @ kcol
    s2 = kss - l @ l
    if not s2 > 0.0:
        raise np.linalg.LinAlgError(f"pivot {N + 1}")
    lnn = np.sqrt(s2)
    v = np.triu(W.T) @ l
    beta = (delta_new - kcol @ alpha) / s2
    Ln = np.zeros((N + 1, N + 1)); Wn = np.zeros((N + 1, N + 1))
    Ln[:N, :N] = L; Ln[N, :N] = l; Ln[N, N] = lnn
    Wn[:N, :N] = W; Wn[N, :N] = -v / lnn; Wn[N, N] = 1.0 / lnn
    return Ln, Wn, np.concatenate([alpha - beta * v, [beta]]), logdet + 2.0 * np.log(lnn), quad + beta * beta * s2


def append_sequential(L, W, alpha, logdet, quad, Kt, delta, N, k):
    """k one-row steps on the dense K̃ (N + k) × (N + k) and its centred targets"""
    st = (L, W, alpha, logdet, quad)
    for i in range(N, N + k):
        st = append_one(*st, Kt[:i, i], Kt[i, i], delta[i])
    return st
