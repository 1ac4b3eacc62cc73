"""numpy restatement of the BatchNorm batch-statistics kernels of csrc/pnpp.hip in the association include/t2h_pnpp.h documents
(every operation rounded once in float32), and their float64 counterparts with the any-order summation bounds the tests
assert.  ``SLAB`` / ``WAVES`` are T2H_BN_SLAB / T2H_BN_WAVES."""
import numpy as np

SLAB, WAVES = 256, 4
F = np.float32
U = 2.0 ** -24                      # unit roundoff of float32


def _seq(terms):
    """Sum of the rows of ``terms`` [n, C] from +0 in ascending order, each addition rounded to float32."""
    acc = np.zeros(terms.shape[1], F)
    if terms.shape[0]:
        acc = np.cumsum(np.concatenate([acc[None], terms]), axis=0, dtype=F)[-1]
    return acc


def col_sum(terms):
    """Column sum of float32 ``terms`` [M, C] in the documented association."""
    terms = np.ascontiguousarray(terms, F)
    total = np.zeros(terms.shape[1], F)
    for r0 in range(0, terms.shape[0], SLAB):
        slab = terms[r0:r0 + SLAB]
        lanes = [_seq(slab[w::WAVES]) for w in range(WAVES)]
        total = total + (((lanes[0] + lanes[1]) + lanes[2]) + lanes[3])
    return total


def col_stats(z, c, eps):
    z = np.asarray(z, F)[:, :c]
    m = F(z.shape[0])
    mean = col_sum(z) / m
    d = z - mean[None]
    var = col_sum(d * d) / m
    rstd = F(1) / np.sqrt(var + F(eps))
    return mean, var, rstd


def apply_relu(z, c, mean, rstd, gamma, beta, ldy):
    z = np.asarray(z, F)[:, :c]
    s = F(gamma) * rstd
    t = F(beta) - mean * s
    y = np.zeros((z.shape[0], ldy), F)
    y[:, :c] = np.maximum(z * s[None] + t[None], F(0))
    return y


def running_update(mean, var, m, momentum, running_mean, running_var):
    keep, mom, mf = F(1) - F(momentum), F(momentum), F(m)
    unbias = mf / (mf - F(1))
    return keep * running_mean + mom * mean, keep * running_var + mom * (var * unbias)


def _masked(gy, y, c, relu):
    g = np.asarray(gy, F)[:, :c].copy()
    if relu:
        g[~(np.asarray(y)[:, :c] > 0)] = 0.0
    return g


def bwd_reduce(gy, y, z, c, mean, rstd, relu):
    g = _masked(gy, y, c, relu)
    xhat = (np.asarray(z, F)[:, :c] - mean[None]) * rstd[None]
    return col_sum(g), col_sum(g * xhat)


def bwd_apply(gy, y, z, c, mean, rstd, gamma, dbeta, dgamma, relu, gld):
    g = _masked(gy, y, c, relu)
    m = F(g.shape[0])
    xhat = (np.asarray(z, F)[:, :c] - mean[None]) * rstd[None]
    a = F(gamma) * rstd
    dz = np.zeros((g.shape[0], gld), F)
    dz[:, :c] = a[None] * ((g - (dbeta / m)[None]) - xhat * (dgamma / m)[None])
    return dz


# ------------------------------------------------------------------------------------------------ float64 and bounds
def sum64(terms32, term_roundings):
    """Float64 column sum of the exact terms' float32 stand-ins and the bound on |kernel sum - exact sum| for ANY summation
    order: (M - 1) u sum|t| for the additions, plus ``term_roundings`` u sum|t| for the roundings inside each term (first
    order, so everything is widened by 1 + 2^-10)."""
    t = np.asarray(terms32, np.float64)
    m = t.shape[0]
    absum = np.abs(t).sum(0)
    return t.sum(0), (m - 1 + term_roundings) * U * absum * (1 + 2.0 ** -10)


def col_stats64(z, c, mean32):
    """(mean64, bound), (var64 about ``mean32``, bound): the variance pass is checked about the mean the kernel itself used (its
    distance to the true variance is (mean32 - mean64)^2, bounded by the first bound squared)."""
    z64 = np.asarray(z, np.float64)[:, :c]
    m = z64.shape[0]
    s, b = sum64(z64, 0)
    mean64, mean_b = s / m, b / m + U * np.abs(s / m) * 2
    d = z64 - np.asarray(mean32, np.float64)[None]
    s, b = sum64(d * d, 3)                     # the difference's rounding twice (squared) and the product's
    return (mean64, mean_b), (s / m, b / m + U * np.abs(s / m) * 2)


def batch_norm64(z, gamma, beta, eps, relu=True):
    """Float64 training-mode BatchNorm (+ ReLU) over rows: (y, mean, biased var)."""
    z = np.asarray(z, np.float64)
    mean, var = z.mean(0), z.var(0)
    y = (z - mean) / np.sqrt(var + eps) * gamma + beta
    return (np.maximum(y, 0) if relu else y), mean, var


def batch_norm_bwd64(gy, z, gamma, eps, y=None):
    """Float64 backward of the above: (dz, dgamma, dbeta); ``y`` given: masked by y > 0 first."""
    z, g = np.asarray(z, np.float64), np.asarray(gy, np.float64).copy()
    if y is not None:
        g[~(np.asarray(y) > 0)] = 0.0
    m = z.shape[0]
    mean, rstd = z.mean(0), 1.0 / np.sqrt(z.var(0) + eps)
    xhat = (z - mean) * rstd
    dbeta, dgamma = g.sum(0), (g * xhat).sum(0)
    return gamma * rstd * (g - dbeta / m - xhat * dgamma / m), dgamma, dbeta
