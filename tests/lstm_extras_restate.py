"""NumPy restatement of csrc/lstm_extras.hip k_lstm_extras_add: dst[r, n] = src[r, n] + sum_x e[r, x] * wx[n, x] in
float32, the accumulator starting at src[r, n] and x ascending, every product and every sum rounded to float32 (the
kernel is built without fused multiply-add).  Shared by the CPU test that holds it to float64 and the GPU test that
holds the kernel to it bit for bit."""
import numpy as np


def extras_add(src, e, wx):
    """src (M, N), e (M, X), wx (N, X), all float32 -> (M, N) float32."""
    src, e, wx = (np.asarray(v, dtype=np.float32) for v in (src, e, wx))
    acc = src.copy()
    for x in range(e.shape[1]):
        prod = (e[:, x:x + 1] * wx[None, :, x]).astype(np.float32)        # float32 * float32 -> rounded float32
        acc = (acc + prod).astype(np.float32)
    return acc


def extras_add_f64(src, e, wx):
    src, e, wx = (np.asarray(v, dtype=np.float64) for v in (src, e, wx))
    return src + e @ wx.T


def extras_add_bound(src, e, wx):
    """(X + 1) 2^-24 (|src| + sum_x |e w|): X products and X sums, each within 2^-24 relative of a partial result that
    is itself bounded by |src| + sum |e w| (to first order; the factor X + 1 instead of X covers the second-order terms)."""
    src, e, wx = (np.asarray(v, dtype=np.float64) for v in (src, e, wx))
    X = e.shape[1]
    return (X + 1) * 2.0 ** -24 * (np.abs(src) + np.abs(e) @ np.abs(wx).T)


def wgrad_f64(g, e):
    """dwx[n, x] = sum_r g[r, n] e[r, x] in float64."""
    return np.asarray(g, dtype=np.float64).T @ np.asarray(e, dtype=np.float64)


def wgrad_bound(g, e):
    """(M + 2) 2^-24 sum_r |g[r, n] e[r, x]|: M products (fused or not) and M - 1 sums in any order."""
    M = np.asarray(g).shape[0]
    return (M + 2) * 2.0 ** -24 * (np.abs(np.asarray(g, dtype=np.float64)).T @ np.abs(np.asarray(e, dtype=np.float64)))


def one_hot_extras(rng, M, X):
    """Rows as ExtraFeaturesEnvWrapper produces them: a one-hot (or all-zero) action block, a small timestep, a reward in
    {-1, 0, 1}; for X < 3 only the action block."""
    e = np.zeros((M, X), np.float32)
    A = X - 2 if X >= 3 else X
    a = rng.integers(-1, A, size=M)
    rows = np.flatnonzero(a >= 0)
    e[rows, a[rows]] = 1.0
    if X >= 3:
        e[:, A] = (rng.integers(0, 5000, size=M).astype(np.float64) * 1e-5).astype(np.float32)
        e[:, A + 1] = rng.integers(-1, 2, size=M).astype(np.float32)
    return e
