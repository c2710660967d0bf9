"""NumPy restatement of abo_remove (csrc/remove.hip; DESIGN.md "Removing an observation"): observation j out of a fitted factor in
O(N²), from L, W = L⁻¹, α, log det and δᵀα alone — in the order the kernels sum in (rows scanned in steps of 64-lane blocks with a
carried running sum; `chunk` = lanes per block) and, for comparison, in plain sequential order (chunk = None).  Test
infrastructure: float64 on the host, no device."""
import numpy as np

CHUNK = 64          # lanes of one scan block (four of them make the REMOVE_SCAN_CHUNK = 256 elements of a kernel step)


def _block_inclusive(v):
    """Hillis–Steele inclusive scan of one block, in lane order: what 64 lanes do with shuffles"""
    v = v.copy()
    o = 1
    while o < len(v):
        t = v.copy()
        t[o:] = v[o:] + v[:-o]
        v = t
        o <<= 1
    return v


def exclusive_scan(v, chunk=CHUNK):
    """ex[e] = Σ_{e' < e} v[e'] — block by block with a carry (chunk lanes), or one sequential running sum (chunk None)"""
    v = np.asarray(v, dtype=np.float64)
    ex = np.zeros_like(v)
    if chunk is None:
        s = 0.0
        for e in range(len(v)):
            ex[e] = s
            s += v[e]
        return ex
    carry = 0.0
    for b in range(0, len(v), chunk):
        blk = np.zeros(chunk)
        n = min(chunk, len(v) - b)
        blk[:n] = v[b:b + n]
        inc = _block_inclusive(blk)
        ex[b:b + n] = carry + np.concatenate([[0.0], inc[:-1]])[:n]
        carry += inc[-1]
    return ex


def coefficients(W, j):
    """p, ρ (m + 1 values), ω of the removal of row j"""
    omega = W[j, j]
    p = -W[j + 1:, j] / omega
    rho = np.sqrt(1.0 + np.concatenate([[0.0], np.cumsum(p * p)]))
    return p, rho, omega


def remove(L, W, alpha, logdet, quad, j, chunk=CHUNK):
    """(L′, W′, α′, log det′, δ′ᵀα′) of the N − 1 remaining observations"""
    N = L.shape[0]
    m = N - 1 - j
    p, rho, omega = coefficients(W, j)
    dl, dw, cc = rho[1:] / rho[:-1], rho[:-1] / rho[1:], p / (rho[:-1] * rho[1:])
    Ln, Wn = np.zeros((N - 1, N - 1)), np.zeros((N - 1, N - 1))
    Ln[:j, :j] = L[:j, :j]
    Wn[:j, :j] = W[:j, :j]
    # L′: row r of the block behind j, a suffix scan (from the diagonal towards column j)
    for kr in range(m):
        r = j + 1 + kr
        Ln[r - 1, :j] = L[r, :j]
        x = L[r, j + 1:r + 1][::-1]                       # position e ↔ column k = kr − e
        pk = p[:kr + 1][::-1]
        ex = exclusive_scan(x * pk, chunk)
        Ln[r - 1, j:r] = (x * dl[:kr + 1][::-1] + cc[:kr + 1][::-1] * ex)[::-1]
    # W′ through the rows of WT (the columns of W), a prefix scan; the same walk gives B[c][j] = (WᵀW)[c][j]
    WT = W.T
    alpha_n = np.zeros(N - 1)
    rho2 = rho[-1] ** 2
    for c in range(N):
        if c == j:
            continue
        cn = c - (c > j)
        w = WT[c, j] if c < j else 0.0
        ks = 0 if c < j else c - j - 1
        x = WT[c, j + 1 + ks:]
        pk = p[ks:]
        mv = x + pk * w
        ex = exclusive_scan(mv * pk, chunk)
        Wn[j + ks:, cn] = dw[ks:] * mv - cc[ks:] * ex
        alpha_n[cn] = alpha[c] - alpha[j] * (w - np.sum(x * pk)) / (omega * rho2)
    bjj = omega * omega * rho2
    return Ln, Wn, alpha_n, logdet + np.log(bjj), quad - alpha[j] ** 2 / bjj


def refit(Kt, delta):
    """(L, W, α, log det, δᵀα) of K̃ = K + σ²I from numpy.linalg"""
    L = np.linalg.cholesky(Kt)
    W = np.linalg.solve(L, np.eye(L.shape[0]))
    W = np.tril(W)
    alpha = W.T @ (W @ delta)
    return L, W, alpha, 2.0 * np.sum(np.log(np.diag(L))), float(delta @ alpha)
