"""numpy restatement of the pgpe strategy (include/ses.h: ses_perturb_mirrored, ses_pgpe_generation) and the float64 reference
of its two sums with the bound the device is held to.  Imports no product code; the normals are the C oracle's Philox normals,
bit-identical to the device's.

Population (bit-exact: one float32 rounding per operation, no fma)
    sig_p = fl(float32(sigma) * scale[p]);  d = fl(sig_p * z_jp);  theta[2j] = fl(mu + d);  theta[2j+1] = fl(mu - d)
with z_j = noise(seed, gen, row = j).

Sums, in float64 here:  Gmu[p] = sum_j d_j z_jp,  Gs[p] = sum_j a_j (z_jp^2 - 1),
    d_j = (w[2j] - w[2j+1]) / 2,  a_j = (w[2j] + w[2j+1]) / 2,  w = the rank-centred weights (stable tie rule).

The bound (pgpe_tolerance), in the form of strategies_np.es_grad_tolerance:
    tol[p] = gamma_K * sum_j |c_j t_jp| + (1 + gamma_K) * WEIGHT_ATOL * sum_j |t_jp|,   gamma_K = K u / (1 - K u), u = 2^-24
with (c, t) = (d, z) for Gmu and (a, z^2 - 1) for Gs.  K counts the float32 roundings one term c_j t_jp can meet on its way
through k_pgpe_grad_partial and k_pgpe_apply (csrc/ses_pgpe.hip):
    1        the cast of the double coefficient d_j / a_j to float32;
    4        the thread's fma chain: thread c of 256 takes the pairs c, c + 256, c + 512, c + 768 of its 1024-pair chunk, a term
             enters at one fma and is rounded by it and by every later one: PGPE_CHUNK / PGPE_THREADS = 4;
    8        the LDS tree over the 256 threads: log2(256) additions;
    chunks   the ordered sum of the chunk partials (chunks - 1 additions; one is spare, as in es_grad_rounding_count);
    +1       for Gs only: the inner fma(z, z, -1) rounds t itself once.
K = 13 + chunks for Gmu, 14 + chunks for Gs (chunks = ceil(n / 2 / 1024)): 14 ... 17 at the sizes the tests use.  The second
term covers the distance between the closed-form weight the device forms and centered_ranks' (WEIGHT_ATOL, per weight; d_j and
a_j are half a sum or difference of two).
"""
import numpy as np

from oracle import c_oracle as co
from oracle import strategies_np as snp

PGPE_CHUNK = 1024          # pairs per gradient workgroup (csrc/ses_pgpe.hip)
PGPE_THREADS = 256
F32_U = 2.0 ** -24
DEFAULTS = dict(sigma_learning_rate=0.2, sigma_max_change=0.2, scale_limits=(0.01, 100.0))


def f32(x):
    return np.asarray(x, dtype=np.float32)


# ---- population ---------------------------------------------------------------------------------------------------------
def population(mu, scale, sigma, seed, gen, first_row=0, n_rows=None, n=None):
    """rows [first_row, first_row + n_rows) of the mirrored population, float32, bit for bit what the device writes"""
    mu, scale = f32(mu), f32(scale)
    P = mu.shape[0]
    if n_rows is None:
        n_rows = n - first_row
    j0, j1 = first_row // 2, (first_row + n_rows - 1) // 2
    z = co.noise(seed, gen, j0, j1 - j0 + 1, P)
    sig = np.float32(sigma) * scale                       # float32 * float32 -> one rounding
    d = sig[None, :] * z
    both = np.empty((2 * (j1 - j0 + 1), P), np.float32)
    both[0::2] = mu[None, :] + d
    both[1::2] = mu[None, :] - d
    lo = first_row - 2 * j0
    return np.ascontiguousarray(both[lo: lo + n_rows])


# ---- weights ------------------------------------------------------------------------------------------------------------
def pair_coefficients(fitness):
    """float64 (d[m], a[m]) from the rank-centred weights of the fitness vector (ties: higher index first)"""
    w = snp.centered_ranks(np.asarray(fitness), stable=True)
    return (w[0::2] - w[1::2]) * 0.5, (w[0::2] + w[1::2]) * 0.5


# ---- float64 sums and their bound -----------------------------------------------------------------------------------------
def pgpe_chunk_sums_f64(d, a, seed, gen, P, noise=None):
    """Per chunk of PGPE_CHUNK pairs: dict of float64 [chunks, P] arrays
    Smu = sum d z, Amu = sum |d z|, Zmu = sum |z|, Ss = sum a (z^2 - 1), As = sum |a (z^2 - 1)|, Zs = sum |z^2 - 1|."""
    noise = co.noise if noise is None else noise
    m = len(d)
    out = {k: [] for k in ("Smu", "Amu", "Zmu", "Ss", "As", "Zs")}
    for c in range(-(-m // PGPE_CHUNK)):
        j0, j1 = c * PGPE_CHUNK, min(m, (c + 1) * PGPE_CHUNK)
        z = noise(seed, gen, j0, j1 - j0, P).astype(np.float64)
        t = z * z - 1.0
        az, at = np.abs(z), np.abs(t)
        out["Smu"].append(d[j0:j1] @ z)
        out["Amu"].append(np.abs(d[j0:j1]) @ az)
        out["Zmu"].append(az.sum(0))
        out["Ss"].append(a[j0:j1] @ t)
        out["As"].append(np.abs(a[j0:j1]) @ at)
        out["Zs"].append(at.sum(0))
    return {k: np.stack(v) for k, v in out.items()}


def pgpe_rounding_count(n, which):
    chunks = -(-(n // 2) // PGPE_CHUNK)
    K = 1 + PGPE_CHUNK // PGPE_THREADS + int(np.log2(PGPE_THREADS)) + chunks
    return K + (1 if which == "s" else 0)


def pgpe_tolerance(n, which, c_abs, t_abs):
    """tol[P] for |G_device - G64|; which = "mu" or "s"; c_abs = sum_j |c_j t_jp|, t_abs = sum_j |t_jp| (float64)"""
    K = pgpe_rounding_count(n, which)
    gamma = K * F32_U / (1.0 - K * F32_U)
    return gamma * c_abs + (1.0 + gamma) * snp.WEIGHT_ATOL * t_abs


def pgpe_sums_f64(fitness, seed, gen, P):
    """(Gmu64, Gs64, tol_mu, tol_s): the float64 sums of a fitness vector and the device's allowance around each"""
    n = len(fitness)
    d, a = pair_coefficients(fitness)
    cs = pgpe_chunk_sums_f64(d, a, seed, gen, P)
    return (cs["Smu"].sum(0), cs["Ss"].sum(0),
            pgpe_tolerance(n, "mu", cs["Amu"].sum(0), cs["Zmu"].sum(0)), pgpe_tolerance(n, "s", cs["As"].sum(0), cs["Zs"].sum(0)))


# ---- the device's summation order in float32 (host emulation) ---------------------------------------------------------------
def emulate_device_sums(d, a, seed, gen, P):
    """float32 (Gmu, Gs) in k_pgpe_grad_partial's and k_pgpe_apply's order.  The fmas are emulated in float64 (the products
    are exact there; the double rounding this may add is far below what is measured)."""
    m = len(d)
    df = d.astype(np.float32).astype(np.float64)
    af = a.astype(np.float32).astype(np.float64)
    tot_mu = tot_s = None
    for c in range(-(-m // PGPE_CHUNK)):
        j0, j1 = c * PGPE_CHUNK, min(m, (c + 1) * PGPE_CHUNK)
        z = np.zeros((PGPE_CHUNK, P))
        z[: j1 - j0] = co.noise(seed, gen, j0, j1 - j0, P)
        t = (z * z - 1.0).astype(np.float32).astype(np.float64)          # fma(z, z, -1): one rounding
        dc, ac = np.zeros(PGPE_CHUNK), np.zeros(PGPE_CHUNK)
        dc[: j1 - j0], ac[: j1 - j0] = df[j0:j1], af[j0:j1]               # rows past the end: coefficient 0, acc unchanged
        z, t = z.reshape(4, PGPE_THREADS, P), t.reshape(4, PGPE_THREADS, P)
        dc, ac = dc.reshape(4, PGPE_THREADS, 1), ac.reshape(4, PGPE_THREADS, 1)
        acc_mu = np.zeros((PGPE_THREADS, P), np.float32)
        acc_s = np.zeros((PGPE_THREADS, P), np.float32)
        for k in range(4):
            acc_mu = (dc[k] * z[k] + acc_mu.astype(np.float64)).astype(np.float32)
            acc_s = (ac[k] * t[k] + acc_s.astype(np.float64)).astype(np.float32)
        s = PGPE_THREADS // 2
        while s:
            acc_mu[:s] = acc_mu[:s] + acc_mu[s:2 * s]
            acc_s[:s] = acc_s[:s] + acc_s[s:2 * s]
            s >>= 1
        tot_mu = acc_mu[0].copy() if tot_mu is None else tot_mu + acc_mu[0]
        tot_s = acc_s[0].copy() if tot_s is None else tot_s + acc_s[0]
    return tot_mu, tot_s


# ---- the update given the two sums ------------------------------------------------------------------------------------------
def grad_mu(Gmu, scale, sigma, n):
    sig = np.float32(sigma) * f32(scale)
    return (f32(Gmu) * sig) * np.float32(-1.0 / (n // 2))


def scale_update(Gs, scale, n, sigma_learning_rate=0.2, sigma_max_change=0.2, scale_limits=(0.01, 100.0)):
    scale = f32(scale)
    cs = np.float32(sigma_learning_rate / (n // 2))
    ds = (f32(Gs) * scale) * cs
    s1 = scale + ds
    lo_f, hi_f = np.float32(1.0 - sigma_max_change), np.float32(1.0 + sigma_max_change)
    s2 = np.minimum(np.maximum(s1, scale * lo_f), scale * hi_f)
    return np.minimum(np.maximum(s2, np.float32(scale_limits[0])), np.float32(scale_limits[1])).astype(np.float32)


def update(mu, m, v, t, scale, Gmu, Gs, sigma, lr, n, **kw):
    """(mu, m, v, scale) after the generation whose sums are (Gmu, Gs); t = Adam steps taken before it"""
    adam = snp.AdamNP(f32(mu).copy(), lr)
    adam.m, adam.v, adam.t = f32(m).copy(), f32(v).copy(), t
    adam.update(grad_mu(Gmu, scale, sigma, n))
    return adam.theta, adam.m, adam.v, scale_update(Gs, scale, n, **kw)


class PgpeNP:
    """The whole strategy on the host (float32 sums in the device's order): what the learning test runs."""

    def __init__(self, P, init_sigma, sigma_decay, learning_rate, offspring_num, seed=0, **kw):
        self.P, self.n, self.seed, self.lr, self.kw = P, offspring_num, seed, learning_rate, {**DEFAULTS, **kw}
        self.curr_sigma, self.sigma_decay = init_sigma, sigma_decay
        self.mu, self.m, self.v, self.t = np.zeros(P, np.float32), np.zeros(P, np.float32), np.zeros(P, np.float32), 0
        self.scale = np.ones(P, np.float32)
        self.gen = 0

    def theta(self):
        return population(self.mu, self.scale, self.curr_sigma, self.seed, self.gen, 0, self.n)

    def evaluate(self, fitness):
        d, a = pair_coefficients(fitness)
        Gmu, Gs = emulate_device_sums(d, a, self.seed, self.gen, self.P)
        self.mu, self.m, self.v, self.scale = update(self.mu, self.m, self.v, self.t, self.scale, Gmu, Gs, self.curr_sigma, self.lr,
                                                     self.n, **self.kw)
        self.t += 1
        self.curr_sigma *= self.sigma_decay
        self.gen += 1
        return float(np.max(fitness))
