"""Float64 yardsticks of the device covariance factor (csrc/padim.hip, ssad_position_gaussian_factor): Higham's componentwise bounds
(Accuracy and Stability of Numerical Algorithms, 2nd ed.), which hold for any summation order in fp64 (u = 2^-53):

 * Cholesky (Theorem 10.3):        |C C^T - Sigma| <= gamma_{d+1} |C| |C|^T,   gamma_k = k u / (1 - k u);
 * substitution (Theorem 8.5 ff.): |W - inv(C)|    <= 2 (d + 1) u |W| |C| |W|, inv(C) from scipy's solve_triangular on the same C
   (half of the bar is that reference's own error of the same form).

The residual C C^T - Sigma is formed in numpy's long double (64-bit significand), so that forming it adds 2^-11 of the bar at most.
Shared by tests/test_padim_factor_host.py and tests/test_hip_padim_factor.py."""
import numpy as np
from scipy.linalg import solve_triangular

U = 2.0 ** -53


def gamma(k):
    return k * U / (1.0 - k * U)


def _worst(err, bound):
    """max err / bound, with 0 / 0 = 0 and x / 0 = inf."""
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0)).max())


def sigma_from_stats(scatter, n, eps):
    """Sigma [P][d][d] = scatter / (n - 1) + eps I in float64, from the LOWER triangle of scatter alone (mirrored)."""
    low = np.tril(np.nan_to_num(np.asarray(scatter, dtype=np.float64), nan=0.0))
    s = low + np.swapaxes(np.tril(low, -1), 1, 2)
    s = s / (n - 1)
    i = np.arange(s.shape[-1])
    s[..., i, i] += eps
    return s


def cholesky_ratio(c, sigma):
    """max over the elements of |C C^T - Sigma| / (gamma_{d+1} |C| |C|^T) for one matrix; <= 1 is the bar."""
    d = c.shape[0]
    assert np.finfo(np.longdouble).eps <= 2.0 ** -60, "this platform's long double is no wider than a double"
    cl = np.tril(c).astype(np.longdouble)
    res = np.abs(cl @ cl.T - sigma.astype(np.longdouble)).astype(np.float64)
    bound = gamma(d + 1) * (np.abs(np.tril(c)) @ np.abs(np.tril(c)).T)
    return _worst(res, bound)


def inverse_ratio(w, c):
    """max over the lower triangle of |W - inv(C)| / (2 (d + 1) u |W| |C| |W|) for one matrix; <= 1 is the bar."""
    d = c.shape[0]
    ref = solve_triangular(np.tril(c), np.eye(d), lower=True)
    aw = np.abs(np.tril(w))
    bound = 2.0 * (d + 1) * U * (aw @ np.abs(np.tril(c)) @ aw)
    low = np.tril_indices(d)
    return _worst(np.abs(np.tril(w) - ref)[low], bound[low])


def factor_model(sigma):
    """(C, W) of one matrix by the textbook recurrences in float64, every element (a - sum_k l_k b_k) / pivot with k ascending: the
    order the kernel keeps (its fused multiply-adds round once where this model rounds twice).  LAPACK-free: a second opinion for the
    bars above."""
    d = sigma.shape[0]
    c = np.zeros((d, d))
    for j in range(d):
        t = sigma[j:, j].copy()
        for k in range(j):
            t -= c[j:, k] * c[j, k]
        piv = t[0]
        if not (piv > 0 and np.isfinite(piv)):
            raise ValueError(f"pivot {j} is not finite and positive")
        c[j, j] = np.sqrt(piv)
        c[j + 1:, j] = t[1:] / c[j, j]
    w = np.zeros((d, d))
    for i in range(d):
        s = np.zeros(d)
        s[i] = 1.0
        for k in range(i):
            s[:i] -= c[i, k] * w[k, :i]
        w[i, :i + 1] = s[:i + 1] / c[i, i]
    return c, w
