"""numpy restatement of the lm_ma_es strategy (include/ses.h: ses_perturb_lmma, ses_lmma_generation), the float64 reference of its
dot products and the bound the device's dots are held to.  Imports no product code; the normals are the C oracle's Philox normals,
bit-identical to the device's.  What lm_ma_es shares with sep_cma_es (the weights and their constants, the weighted sum Sz with its
order and bound, p_sigma', norm2) is taken from tests/sep_cma_np.py.

Constants (double, from (n, P, mu, m); mu = the number of selected rows, default n // 2; m = the direction vectors, default
min(32, 4 + floor(3 ln P)))
    w_k, mueff, c_sigma, d_sigma, chi: sep_cma_np.constants
    c_d[j] = 1 / (1.5^j P),  c_c[j] = min(1, n / (4^j P)),  j < m
    float32 tables: cd = c_d, ad = 1 - c_d, ac = 1 - c_c, bc = sqrt(mueff c_c (2 - c_c))

Population (bit-exact GIVEN the dots: one float32 rounding per operation, no fma outside the dots)
    v_0 = z_i = noise(seed, gen, row = i);  for j < m_active:  v_{j+1} = fl(fl(ad[j] v_j) + fl(fl(cd[j] dot_j) M[j]))
    theta[i] = fl(mu + fl(fl(float32(sigma) * step) * v_last))

The dot of a row, dot_j = sum_p M[j][p] v_j[p], in the device's order (dot_device_order; k_perturb_lmma of csrc/ses_lmma.hip): T = 64
threads for P <= 256 and 256 above; thread c owns the quads q = c, c + T, ...; four fma chains per thread (one per position inside
a quad, over the thread's quads in ascending order), x = (a_0 + a_1) + (a_2 + a_3), a butterfly over the 64 lanes of each wave
(x[l] += x[l ^ s], s = 32 ... 1), and for T = 256 a butterfly over the four wave sums (s = 2, 1).

The bound (dot_tolerance), in the form of sepcma_tolerance:
    tol = gamma_K * sum_p |M[j][p] v_j[p]|,   gamma_K = K u / (1 - K u), u = 2^-24
K counts the float32 roundings one product can meet on its way (the products themselves are exact inside the fma):
    R        the thread's chain, R = ceil(ceil(P / 4) / T) fmas: a term is rounded by the fma it enters at and by every later one;
    2        (a_0 + a_1) + (a_2 + a_3);
    6        the butterfly over 64 lanes;
    log2(W)  the butterfly over the W = T / 64 wave sums.
K = 9 at P = 226, 11 at P = 581, 17 at P = 6562.  The update's dot sdot_j = sum_p M[j][p] u_j[p] (k_lmma_update: thread c of 1024
takes p = c, c + 1024, ... as one fma chain, the 64-lane butterfly, a butterfly over the 16 wave sums) has K = ceil(P / 1024) + 6 + 4.
"""
import math

import numpy as np

import sep_cma_np as sc
from oracle import c_oracle as co

F32_U = 2.0 ** -24
UPDATE_THREADS = 1024
MAX_MEMORY = 32
DEFAULT_STEP_LIMITS = (1e-6, 1e6)


def f32(x):
    return np.asarray(x, dtype=np.float32)


# ---- constants ------------------------------------------------------------------------------------------------------------
def default_memory(P):
    return min(MAX_MEMORY, 4 + int(math.floor(3.0 * math.log(P))))


def constants(n, P, mu=None, m=None):
    """(dict of the doubles + mu + m + the lists c_d, c_c; float32 weights[mu])"""
    c, w = sc.constants(n, P, mu)
    m = default_memory(P) if m is None else int(m)
    c_d = [1.0 / (1.5 ** j * P) for j in range(m)]
    c_c = [min(1.0, n / (4.0 ** j * P)) for j in range(m)]
    return dict(mu=c["mu"], m=m, mueff=c["mueff"], c_sigma=c["c_sigma"], d_sigma=c["d_sigma"], chi=c["chi"], c_d=c_d, c_c=c_c), w


def tables(c):
    """the four float32 tables the kernels read, each entry cast from double once"""
    cd = np.array(c["c_d"], np.float64)
    cc = np.array(c["c_c"], np.float64)
    return dict(cd=cd.astype(np.float32), ad=(1.0 - cd).astype(np.float32), ac=(1.0 - cc).astype(np.float32),
                bc=np.sqrt(c["mueff"] * cc * (2.0 - cc)).astype(np.float32))


# ---- the dots ---------------------------------------------------------------------------------------------------------------
def threads(P):
    return 64 if P <= 256 else 256


def _butterfly(x, width):
    """x[..., l] + x[..., l ^ s] for s = width / 2 ... 1 over the last axis (length = width), float32"""
    idx = np.arange(width)
    s = width // 2
    while s:
        x = x + x[..., idx ^ s]
        s >>= 1
    return x


def _fma32(a, b, acc):
    """float32 fma emulated in float64: the product is exact there (the double rounding this may add is far below any bound)"""
    return (a.astype(np.float64) * b.astype(np.float64) + acc.astype(np.float64)).astype(np.float32)


def dot_device_order(Mj, v):
    """float32 dots of the rows of v[rows, P] (or one vector v[P]) with Mj[P], in k_perturb_lmma's order"""
    Mj, v = f32(Mj), f32(v)
    one = v.ndim == 1
    v = np.atleast_2d(v)
    rows, P = v.shape
    T = threads(P)
    quads = -(-P // 4)
    R = -(-quads // T)
    Mp = np.zeros(R * T * 4, np.float32)
    Mp[:P] = Mj
    vp = np.zeros((rows, R * T * 4), np.float32)
    vp[:, :P] = v
    Mp, vp = Mp.reshape(R, T, 4), vp.reshape(rows, R, T, 4)
    acc = np.zeros((rows, T, 4), np.float32)
    for r in range(R):
        acc = _fma32(np.broadcast_to(Mp[r], acc.shape), vp[:, r], acc)
    x = (acc[..., 0] + acc[..., 1]) + (acc[..., 2] + acc[..., 3])
    W = T // 64
    x = _butterfly(x.reshape(rows, W, 64), 64)[:, :, 0]
    out = _butterfly(x, W)[:, 0]
    return out[0] if one else out


def sdot_device_order(Mj, u):
    """the float32 dot of u[P] with Mj[P] in k_lmma_update's order"""
    Mj, u = f32(Mj), f32(u)
    P = u.shape[0]
    R = -(-P // UPDATE_THREADS)
    Mp, up = np.zeros(R * UPDATE_THREADS, np.float32), np.zeros(R * UPDATE_THREADS, np.float32)
    Mp[:P], up[:P] = Mj, u
    Mp, up = Mp.reshape(R, UPDATE_THREADS), up.reshape(R, UPDATE_THREADS)
    acc = np.zeros(UPDATE_THREADS, np.float32)
    for r in range(R):
        acc = _fma32(Mp[r], up[r], acc)
    x = _butterfly(acc.reshape(16, 64), 64)[:, 0]
    return _butterfly(x, 16)[0]


def dot_f64(Mj, v):
    """the float64 dots of the rows of v (float32 values) with Mj"""
    return f32(v).astype(np.float64) @ f32(Mj).astype(np.float64)


def dot_rounding_count(P):
    T = threads(P)
    return -(-(-(-P // 4)) // T) + 2 + 6 + int(np.log2(T // 64))


def sdot_rounding_count(P):
    return -(-P // UPDATE_THREADS) + 6 + 4


def _gamma(K):
    return K * F32_U / (1.0 - K * F32_U)


def dot_tolerance(Mj, v):
    """tol[rows] for |dot_device - dot64| of the rows of v with Mj (k_perturb_lmma's order)"""
    Mj, v = f32(Mj).astype(np.float64), f32(v).astype(np.float64)
    return _gamma(dot_rounding_count(Mj.shape[0])) * (np.abs(v) @ np.abs(Mj))


def sdot_tolerance(Mj, u):
    Mj, u = f32(Mj).astype(np.float64), f32(u).astype(np.float64)
    return _gamma(sdot_rounding_count(Mj.shape[0])) * float(np.abs(u) @ np.abs(Mj))


# ---- the transform ----------------------------------------------------------------------------------------------------------
def transform_step(v, Mj, dot, j, tab):
    """v_{j+1} = fl(fl(ad[j] v) + fl(fl(cd[j] dot) Mj)), elementwise in float32; v[rows, P] with dot[rows], or v[P] with a scalar"""
    v, Mj = f32(v), f32(Mj)
    g = tab["cd"][j] * f32(dot)
    if v.ndim == 2:
        g = g[:, None]
        Mj = Mj[None, :]
    out = tab["ad"][j] * v + g * Mj
    assert out.dtype == np.float32
    return out


def transform_f64(x, M, c, m_active):
    """the transform in exact-ish arithmetic: float64, the double constants; x[..., P]"""
    x = np.asarray(x, np.float64)
    for j in range(m_active):
        Mj = np.asarray(M[j], np.float64)
        x = (1.0 - c["c_d"][j]) * x + c["c_d"][j] * (x @ Mj)[..., None] * Mj
    return x


def population(mu, M, step, sigma, seed, gen, tab, m_active, first_row=0, n_rows=None, n=None, dots=None, chain=False):
    """rows [first_row, first_row + n_rows) of the population, float32.  dots[n_rows, m_active]: the dots to use (the device's:
    the result is then bit for bit what the device writes); None: they are formed here in the device's order.  Returns (theta,
    dots used), or (theta, dots used, [v_0, ..., v_{m_active - 1}]: the vector each dot was taken of) with chain."""
    mu = f32(mu)
    if n_rows is None:
        n_rows = n - first_row
    v = co.noise(seed, gen, first_row, n_rows, mu.shape[0])
    used = np.zeros((n_rows, m_active), np.float32)
    vs = []
    for j in range(m_active):
        vs.append(v)
        used[:, j] = dot_device_order(M[j], v) if dots is None else f32(dots)[:, j]
        v = transform_step(v, M[j], used[:, j], j, tab)
    s0 = np.float32(sigma) * np.float32(step)             # float32 * float32 -> one rounding
    theta = np.ascontiguousarray(mu[None, :] + s0 * v)
    assert theta.dtype == np.float32
    return (theta, used, vs) if chain else (theta, used)


# ---- Sz in the device's order ---------------------------------------------------------------------------------------------------
def sz_device_order(w, seed, gen, P):
    """float32 Sz in k_sepcma_sums_partial's and the update's order, as sep_cma_np.emulate_device_sums forms it (the same bits),
    without the Szz half and visiting, like the kernel, only the rows that carry a weight"""
    n = len(w)
    wf = w.astype(np.float32)
    tot = None
    for c in range(-(-n // sc.CHUNK)):
        i0, i1 = c * sc.CHUNK, min(n, (c + 1) * sc.CHUNK)
        z = co.noise(seed, gen, i0, i1 - i0, P)
        acc = np.zeros((sc.THREADS, P), np.float32)
        for k in range(sc.CHUNK // sc.THREADS):
            rows = np.arange(k * sc.THREADS, min((k + 1) * sc.THREADS, i1 - i0))
            rows = rows[wf[i0 + rows] != 0]
            if len(rows):
                t = rows - k * sc.THREADS
                acc[t] = _fma32(wf[i0 + rows][:, None], z[rows], acc[t])
        s = sc.THREADS // 2
        while s:
            acc[:s] = acc[:s] + acc[s:2 * s]
            s >>= 1
        tot = acc[0].copy() if tot is None else tot + acc[0]
    return tot


# ---- the update given (Sz, sdots, norm2) ----------------------------------------------------------------------------------------
def step_update(norm2, step, c, step_limits=DEFAULT_STEP_LIMITS):
    """step' from norm2, in double as the one thread of k_lmma_update computes it; rounded and clamped in float32"""
    e = (c["c_sigma"] / c["d_sigma"]) * (math.sqrt(norm2) / c["chi"] - 1.0)
    capped = e > 1.0
    if capped:
        e = 1.0
    sn = np.float32(float(np.float32(step)) * math.exp(e))
    out = np.minimum(np.maximum(sn, np.float32(step_limits[0])), np.float32(step_limits[1]))
    return np.float32(out), dict(exponent=e, capped=capped, unclamped=sn)


def mean_chain(Sz, M, tab, m_active, sdots=None):
    """(u_last, sdots used, [u_0, ..., u_{m_active - 1}]): the transform applied to Sz with the dots given (the device's) or formed
    here in k_lmma_update's order"""
    u = f32(Sz)
    used = np.zeros(m_active, np.float32)
    us = []
    for j in range(m_active):
        us.append(u)
        used[j] = sdot_device_order(M[j], u) if sdots is None else f32(sdots)[j]
        u = transform_step(u, M[j], used[j], j, tab)
    return u, used, us


def update(mu, ps, M, step, Sz, sdots, norm2, sigma, c, tab, m_active, step_limits=DEFAULT_STEP_LIMITS):
    """((mu, p_sigma, M, step)', info) after the generation whose weighted sum is Sz, whose mean chain met the dots sdots (None:
    formed here) and whose |p_sigma'|^2 is norm2; one numpy float32 operation per device operation.  sigma: the curr_sigma the
    evaluated population was drawn with; m_active: the vectors it was drawn with."""
    mu, ps, M, Sz = f32(mu), f32(ps), f32(M), f32(Sz)
    ps_new = sc.path_sigma(ps, Sz, c)
    step_new, info = step_update(norm2, step, c, step_limits)
    u_last, used, us = mean_chain(Sz, M, tab, m_active, sdots)
    mu_new = mu + (np.float32(sigma) * np.float32(step)) * u_last
    M_new = tab["ac"][:, None] * M + tab["bc"][:, None] * Sz[None, :] if c["m"] else M.copy()
    assert mu_new.dtype == np.float32 and M_new.dtype == np.float32
    info.update(u_last=u_last, sdots=used, chain=us)
    return (mu_new, ps_new, M_new, step_new), info


class LmMaNP:
    """The whole strategy on the host (float32 sums and dots in the device's orders): what the learning tests run."""

    def __init__(self, P, init_sigma, sigma_decay, offspring_num, elite_num=None, memory=None, seed=0, step_limits=DEFAULT_STEP_LIMITS):
        self.P, self.n, self.seed, self.step_limits = P, offspring_num, seed, step_limits
        self.c, self.weights = constants(offspring_num, P, elite_num, memory)
        self.tab = tables(self.c)
        self.curr_sigma, self.sigma_decay = init_sigma, sigma_decay
        self.mu, self.ps = np.zeros(P, np.float32), np.zeros(P, np.float32)
        self.M = np.zeros((self.c["m"], P), np.float32)
        self.step = np.float32(1.0)
        self.t = 0
        self.gen = 0

    @property
    def m_active(self):
        return min(self.t, self.c["m"])

    def theta(self):
        return population(self.mu, self.M, self.step, self.curr_sigma, self.seed, self.gen, self.tab, self.m_active, 0, self.n)[0]

    def evaluate(self, fitness):
        w = sc.row_weights(fitness, self.weights)
        Sz = sz_device_order(w, self.seed, self.gen, self.P)
        norm2 = sc.norm2_device_order(sc.path_sigma(self.ps, Sz, self.c))
        (self.mu, self.ps, self.M, self.step), _ = update(self.mu, self.ps, self.M, self.step, Sz, None, norm2, self.curr_sigma,
                                                          self.c, self.tab, self.m_active, self.step_limits)
        self.t += 1
        self.curr_sigma *= self.sigma_decay
        self.gen += 1
        return float(np.max(fitness))
