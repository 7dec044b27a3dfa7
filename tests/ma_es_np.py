"""numpy restatement of the ma_es strategy (include/ses.h: ses_perturb_maes, ses_maes_generation), the float64 reference of its
products and the bound the device's products are held to.  Imports no product code; the normals are the C oracle's Philox normals,
bit-identical to the device's.  What ma_es shares with sep_cma_es and lm_ma_es (the weights and their constants, the weighted sum Sz
with its order, p_sigma', norm2, the step) is taken from tests/sep_cma_np.py and tests/lm_ma_np.py.

Constants (double, from (n, P, mu); mu = the number of selected rows, default n // 2)
    w_k, mueff, c_sigma, d_sigma, chi: sep_cma_np.constants
    c_1 = 2 / ((P + 1.3)^2 + mueff),  c_mu = min(1 - c_1, 2 (mueff - 2 + 1 / mueff) / ((P + 2)^2 + mueff))
    float32: a_m = 1 - c_1 / 2 - c_mu / 2,  c1h = c_1 / 2,  cmuh = c_mu / 2

Population GIVEN D (bit-exact: one float32 rounding per operation)
    theta[i] = fl(mu + fl(fl(float32(sigma) * step) * D[i]))
Update GIVEN (Sz, Sd, qv, G, norm2) (bit-exact likewise)
    p_sigma' = fl(fl(a_s p_sigma) + fl(b_s Sz));  step' from norm2 (lm_ma_np.step_update);  mu' = fl(mu + fl(fl(sigma step) Sd))
    M'[p][q] = fl(fl(fl(a_m M[p][q]) + fl(c1h fl(qv[p] p_sigma'[q]))) + fl(cmuh G[p][q]))

The products in the device's orders (what the host-only strategy MaEsNP runs on):
    D[i][p]   one chain acc = fma(z_i[q], M[p][q], acc) from +0 over q = 0 .. P - 1                           (d_device_order)
    Sd, qv    64 chains, chain l over q = l, l + 64, ... from +0, then a butterfly y[l] += y[l ^ s], s = 32 ... 1    (matvec_device_order)
    G[p][q]   one chain acc = fma(fl(w_i D[i][p]), z_i[q], acc) from +0 over the selected rows in ascending row index  (g_device_order)
An odd chain length is padded with one fma(+0, +0, acc): it changes no value (at most the sign of a zero).

The bound (product_tolerance), in the form of lm_ma_np.dot_tolerance:
    tol = gamma_K * sum_k |a_k| |b_k|,   gamma_K = K u / (1 - K u), u = 2^-24
K counts the float32 roundings one product can meet on its way (the products themselves are exact inside the fma):
    D         K = P:  a term is rounded by the fma it enters at and by every later one of the chain
    Sd, qv    K = ceil(P / 64) + 6:  the lane's chain and the butterfly over 64 lanes
    G         K = mu + 1:  the chain over the mu selected rows, and the rounding of fl(w_i D[i][p]) before it
"""
import numpy as np

import lm_ma_np as lm
import sep_cma_np as sc
from oracle import c_oracle as co

F32_U = 2.0 ** -24
MAX_P = 1024
DEFAULT_STEP_LIMITS = (1e-6, 1e6)
f32 = sc.f32


def _fma32(a, b, acc):
    """float32 fma, exact: the product of two float32 is exact in float64; the sum with acc is formed there with its rounding
    error (TwoSum), rounded to ODD where it is inexact, and only then to float32 -- round-to-odd at 53 bits followed by
    round-to-nearest at 24 is the correctly rounded result, so a chain of these is the device's chain bit for bit"""
    p = np.asarray(a, np.float32).astype(np.float64) * np.asarray(b, np.float32).astype(np.float64)
    c = np.asarray(acc, np.float32).astype(np.float64)
    p, c = np.broadcast_arrays(p, c)
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    fix = (err != 0.0) & ((s.view(np.int64) & 1) == 0)
    if fix.any():
        s = np.where(fix, np.nextafter(s, np.where(err > 0.0, np.inf, -np.inf)), s)
    return s.astype(np.float32)


# ---- constants ------------------------------------------------------------------------------------------------------------
def constants(n, P, mu=None):
    """(dict of the doubles + mu; float32 weights[mu])"""
    c, w = sc.constants(n, P, mu)
    mueff = c["mueff"]
    c_1 = 2.0 / ((P + 1.3) ** 2 + mueff)
    c_mu = min(1.0 - c_1, 2.0 * (mueff - 2.0 + 1.0 / mueff) / ((P + 2.0) ** 2 + mueff))
    return dict(mu=c["mu"], mueff=mueff, c_sigma=c["c_sigma"], d_sigma=c["d_sigma"], chi=c["chi"], c_1=c_1, c_mu=c_mu), w


def factors(c):
    """(a_m, c1h, cmuh): the three float32 factors of the matrix update, each cast from double once"""
    return np.float32(1.0 - c["c_1"] / 2.0 - c["c_mu"] / 2.0), np.float32(c["c_1"] / 2.0), np.float32(c["c_mu"] / 2.0)


# ---- the products in the device's orders ---------------------------------------------------------------------------------------
def d_device_order(M, z):
    """float32 D[rows, P] = z M^T: one fma chain per element, q ascending from +0"""
    M, z = f32(M), f32(z)
    acc = np.zeros((z.shape[0], M.shape[0]), np.float32)
    for q in range(M.shape[1]):
        acc = _fma32(z[:, q:q + 1], M[None, :, q], acc)
    return acc


def matvec_device_order(M, x):
    """float32 M x: per row 64 chains (chain l over q = l, l + 64, ...), then the butterfly over the 64 chains"""
    M, x = f32(M), f32(x)
    P = M.shape[1]
    R = -(-P // 64)
    Mp, xp = np.zeros((M.shape[0], R * 64), np.float32), np.zeros(R * 64, np.float32)
    Mp[:, :P], xp[:P] = M, x
    acc = np.zeros((M.shape[0], 64), np.float32)
    for r in range(R):
        acc = _fma32(Mp[:, 64 * r:64 * r + 64], xp[None, 64 * r:64 * r + 64], acc)
    return lm._butterfly(acc, 64)[:, 0]


def selected_rows(w):
    """the rows that carry a weight, in ascending row index"""
    return np.flatnonzero(np.asarray(w) != 0)


def g_device_order(w, D, z):
    """float32 G[P, P] = sum over the selected rows i (ascending) of fl(w_i D[i][p]) z_i[q]: one fma chain per element from +0.
    w[n]: the row weights (0 = not selected); D, z: [n, P]"""
    D, z = f32(D), f32(z)
    wf = np.asarray(w).astype(np.float32)
    acc = np.zeros((D.shape[1], z.shape[1]), np.float32)
    for i in selected_rows(w):
        a = wf[i] * D[i]
        assert a.dtype == np.float32
        acc = _fma32(a[:, None], z[i][None, :], acc)
    return acc


# ---- float64 references and the bound ---------------------------------------------------------------------------------------------
def _gamma(K):
    return K * F32_U / (1.0 - K * F32_U)


def product_tolerance(abs_a, abs_b, K):
    """gamma_K * |a| . |b| for every element of the product a @ b (abs_a[r, k], abs_b[k, c]: float64, already absolute)"""
    return _gamma(K) * (np.asarray(abs_a, np.float64) @ np.asarray(abs_b, np.float64))


def d_f64(M, z):
    return f32(z).astype(np.float64) @ f32(M).astype(np.float64).T


def d_tolerance(M, z):
    """tol[rows, P] for |D_device - D64|"""
    M = f32(M)
    return product_tolerance(np.abs(f32(z)), np.abs(M).T, M.shape[1])


def matvec_f64(M, x):
    return f32(M).astype(np.float64) @ f32(x).astype(np.float64)


def matvec_rounding_count(P):
    return -(-P // 64) + 6


def matvec_tolerance(M, x):
    M = f32(M)
    return product_tolerance(np.abs(M), np.abs(f32(x)), matvec_rounding_count(M.shape[1]))


def g_f64(w, D, z):
    """sum_i w_i D[i][p] z_i[q] in float64, w_i the float32 weight (the product w_i D[i][p] NOT rounded)"""
    rows = selected_rows(w)
    wd = np.asarray(w).astype(np.float32).astype(np.float64)[rows, None] * f32(D).astype(np.float64)[rows]
    return wd.T @ f32(z).astype(np.float64)[rows]


def g_tolerance(w, D, z):
    rows = selected_rows(w)
    wd = np.asarray(w).astype(np.float32).astype(np.float64)[rows, None] * f32(D).astype(np.float64)[rows]
    return product_tolerance(np.abs(wd).T, np.abs(f32(z)[rows]), len(rows) + 1)


# ---- the population given D, the update given the products ----------------------------------------------------------------------
def population(mu, step, sigma, D):
    """theta = fl(mu + fl(fl(float32(sigma) * step) * D)), float32, bit for bit what the device writes for that D"""
    s0 = np.float32(sigma) * np.float32(step)              # float32 * float32 -> one rounding
    theta = np.ascontiguousarray(f32(mu)[None, :] + s0 * f32(D))
    assert theta.dtype == np.float32
    return theta


def update(mu, ps, M, step, Sz, Sd, qv, G, norm2, sigma, c, step_limits=DEFAULT_STEP_LIMITS):
    """((mu, p_sigma, M, step)', info) after the generation whose weighted sum is Sz, whose products with the old M are Sd = M Sz and
    qv = M p_sigma', whose selected rows give G and whose |p_sigma'|^2 is norm2; one numpy float32 operation per device operation.
    sigma: the curr_sigma the evaluated population was drawn with."""
    mu, ps, M, Sz, Sd, qv, G = (f32(x) for x in (mu, ps, M, Sz, Sd, qv, G))
    a_m, c1h, cmuh = factors(c)
    ps_new = sc.path_sigma(ps, Sz, c)
    step_new, info = lm.step_update(norm2, step, c, step_limits)
    mu_new = mu + (np.float32(sigma) * np.float32(step)) * Sd
    M_new = (a_m * M + c1h * (qv[:, None] * ps_new[None, :])) + cmuh * G
    assert mu_new.dtype == np.float32 and M_new.dtype == np.float32
    return (mu_new, ps_new, M_new, step_new), info


class MaEsNP:
    """The whole strategy on the host (float32 sums and products in the device's orders): what the learning tests run."""

    def __init__(self, P, init_sigma, sigma_decay, offspring_num, elite_num=None, seed=0, step_limits=DEFAULT_STEP_LIMITS):
        if P > MAX_P:
            raise ValueError(f"ma_es serves up to {MAX_P} parameters")
        self.P, self.n, self.seed, self.step_limits = P, offspring_num, seed, step_limits
        self.c, self.weights = constants(offspring_num, P, elite_num)
        self.curr_sigma, self.sigma_decay = init_sigma, sigma_decay
        self.mu, self.ps = np.zeros(P, np.float32), np.zeros(P, np.float32)
        self.M = np.eye(P, dtype=np.float32)
        self.step = np.float32(1.0)
        self.t = 0
        self.gen = 0
        self.D = None

    def theta(self):
        self.D = d_device_order(self.M, co.noise(self.seed, self.gen, 0, self.n, self.P))
        return population(self.mu, self.step, self.curr_sigma, self.D)

    def evaluate(self, fitness):
        if self.D is None:
            self.theta()
        w = sc.row_weights(fitness, self.weights)
        Sz = lm.sz_device_order(w, self.seed, self.gen, self.P)
        ps_new = sc.path_sigma(self.ps, Sz, self.c)
        norm2 = sc.norm2_device_order(ps_new)
        Sd, qv = matvec_device_order(self.M, Sz), matvec_device_order(self.M, ps_new)
        G = g_device_order(w, self.D, co.noise(self.seed, self.gen, 0, self.n, self.P))
        (self.mu, self.ps, self.M, self.step), _ = update(self.mu, self.ps, self.M, self.step, Sz, Sd, qv, G, norm2, self.curr_sigma,
                                                          self.c, self.step_limits)
        self.t += 1
        self.curr_sigma *= self.sigma_decay
        self.gen += 1
        self.D = None
        return float(np.max(fitness))
