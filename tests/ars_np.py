"""numpy restatement of the ars strategy (include/ses.h: ses_ars_generation) and the float64 reference of its sum with the bound the
device is held to.  Imports no product code; the normals are the C oracle's Philox normals, bit-identical to the device's.

Population (bit-exact: one float32 rounding per operation, no fma)
    d = fl(float32(sigma) * z_jp);  theta[2j] = fl(mu + d);  theta[2j+1] = fl(mu - d),  z_j = noise(seed, gen, row = j)
which is pgpe_np.population with scale = 1.

Selection (bit-exact).  s_j = max(f[2j], f[2j+1]); rank[j] = #{ i : s_i > s_j or (s_i == s_j and i > j) } -- the tie rule of
ses_rank_center, restated: among equal scores the HIGHER pair index comes first; sel_k = the pair of rank k, k < b.

sigma_R (bit-exact, double).  The 2 b values x_e = f[2 sel_{e // 2} + (e & 1)]: thread c of 256 adds x_c, x_{c + 256}, ... in
ascending order to 0.0, an 8-level tree x[c] += x[c + s], s = 128 ... 1, adds the threads; mean = sum / (2 b); the squared
deviations (x_e - mean)^2, product and sum rounded separately, are added in the same order; sigma_R = sqrt(sum / (2 b)).

Sum.  d_k = float32(float64(f[2 sel_k]) - float64(f[2 sel_k + 1])),  G[p] = sum_k d_k z_{sel_k, p};  in float64 here (the float64
reference keeps the exact double difference), and emulated in the device's float32 order (emulate_device_sum).

The bound (ars_tolerance), in the form of pgpe_np.pgpe_tolerance without its weight term (the coefficient is a difference of two
given float32 values, exact in double: there is no closed-form weight to differ from):
    tol[p] = gamma_K * sum_k |d_k z_{sel_k, p}|,   gamma_K = K u / (1 - K u), u = 2^-24
K counts the float32 roundings one term can meet on its way through k_ars_grad_partial and the update (csrc/ses_ars.hip):
    1        the cast of the double difference d_k to float32;
    4        the thread's fma chain: thread c of 256 takes k = c, c + 256, c + 512, c + 768 of its chunk of 1024 selected pairs, a
             term enters at one fma and is rounded by it and by every later one: ARS_CHUNK / ARS_THREADS = 4;
    8        the LDS tree over the 256 threads: log2(256) additions;
    chunks   the ordered sum of the chunk partials (chunks - 1 additions; one is spare, as in pgpe_rounding_count).
K = 13 + chunks, chunks = ceil(b / 1024): 14 or 15 at the sizes the tests use.  With every difference zero the bound is zero and so
is the sum, exactly.

Update (bit-exact given G):  step = float32(learning_rate / (b * sigma_R)) if sigma_R > 0 else 0;  mu' = fl(mu + fl(step * G)).
"""
import numpy as np

from oracle import c_oracle as co

ARS_CHUNK = 1024           # selected pairs per gradient workgroup (csrc/ses_ars.hip)
ARS_THREADS = 256
F32_U = 2.0 ** -24


def f32(x):
    return np.asarray(x, dtype=np.float32)


# ---- population ---------------------------------------------------------------------------------------------------------
def population(mu, sigma, seed, gen, first_row=0, n_rows=None, n=None):
    """rows [first_row, first_row + n_rows) of the mirrored population, float32, bit for bit what the device writes"""
    mu = f32(mu)
    P = mu.shape[0]
    if n_rows is None:
        n_rows = n - first_row
    j0, j1 = first_row // 2, (first_row + n_rows - 1) // 2
    d = np.float32(sigma) * co.noise(seed, gen, j0, j1 - j0 + 1, P)
    both = np.empty((2 * (j1 - j0 + 1), P), np.float32)
    both[0::2] = mu[None, :] + d
    both[1::2] = mu[None, :] - d
    lo = first_row - 2 * j0
    return np.ascontiguousarray(both[lo: lo + n_rows])


# ---- selection ----------------------------------------------------------------------------------------------------------
def pair_scores(fitness):
    fitness = f32(fitness)
    return np.maximum(fitness[0::2], fitness[1::2])


def rank_pairs(scores):
    """rank[j] = #{ i : s_i > s_j or (s_i == s_j and i > j) } as int64[m]"""
    m = len(scores)
    order = np.lexsort((-np.arange(m), -np.asarray(scores, np.float64)))     # by score descending, then by index descending
    rank = np.empty(m, np.int64)
    rank[order] = np.arange(m)
    return rank


def select(fitness, b):
    """sel[b]: the pairs of rank 0 .. b - 1, in rank order"""
    rank = rank_pairs(pair_scores(fitness))
    sel = np.empty(len(rank), np.int64)
    sel[rank] = np.arange(len(rank))
    return sel[:b]


# ---- sigma_R ------------------------------------------------------------------------------------------------------------
def _ordered_sum(x):
    """float64 sum of x in the device's order: 256 strided running sums from 0.0, then the 8-level tree"""
    pad = (-len(x)) % ARS_THREADS
    rows = np.concatenate([np.asarray(x, np.float64), np.zeros(pad)]).reshape(-1, ARS_THREADS)
    acc = np.zeros(ARS_THREADS)
    for r in rows:
        acc = acc + r
    s = ARS_THREADS // 2
    while s:
        acc[:s] = acc[:s] + acc[s:2 * s]
        s >>= 1
    return acc[0]


def kept_returns(fitness, sel):
    fitness = f32(fitness)
    x = np.empty(2 * len(sel), np.float64)
    x[0::2], x[1::2] = fitness[2 * sel], fitness[2 * sel + 1]
    return x


def sigma_r(fitness, sel, divisor=None):
    """the population standard deviation of the 2 b kept returns, float64, bit for bit the device's"""
    x = kept_returns(fitness, sel)
    count = float(len(x) if divisor is None else divisor)
    mean = _ordered_sum(x) / count
    dv = x - mean
    return float(np.sqrt(_ordered_sum(dv * dv) / count))


# ---- the sum: float64, its bound, the device's float32 order ----------------------------------------------------------------
def differences(fitness, sel):
    """(d64[b], d32[b]): the exact double differences of the selected pairs and what the device multiplies with"""
    fitness = f32(fitness).astype(np.float64)
    d64 = fitness[2 * sel] - fitness[2 * sel + 1]
    return d64, d64.astype(np.float32)


def selected_noise(sel, seed, gen, P):
    """float32 z[b, P]: the noise rows of the selected pairs, in rank order"""
    sel = np.asarray(sel, np.int64)
    lo, hi = int(sel.min()), int(sel.max())
    return co.noise(seed, gen, lo, hi - lo + 1, P)[sel - lo]


def ars_rounding_count(b):
    chunks = -(-b // ARS_CHUNK)
    return 1 + ARS_CHUNK // ARS_THREADS + int(np.log2(ARS_THREADS)) + chunks


def ars_tolerance(b, term_abs):
    """tol[P] for |G_device - G64|; term_abs = sum_k |d_k z_{sel_k, p}| (float64)"""
    K = ars_rounding_count(b)
    return K * F32_U / (1.0 - K * F32_U) * term_abs


def ars_sum_f64(d64, z):
    """(G64[P], tol[P]) of coefficients d64[b] on noise rows z[b, P]"""
    z = z.astype(np.float64)
    return d64 @ z, ars_tolerance(len(d64), np.abs(d64) @ np.abs(z))


def ars_reference(fitness, b, seed, gen, P):
    """(sel, sigma_R, G64, tol) of a fitness vector: everything the device's results are compared with"""
    sel = select(fitness, b)
    d64, _ = differences(fitness, sel)
    g64, tol = ars_sum_f64(d64, selected_noise(sel, seed, gen, P))
    return sel, sigma_r(fitness, sel), g64, tol


def emulate_device_sum(d32, z):
    """float32 G in k_ars_grad_partial's and the update's order.  The fmas are emulated in float64 (the products are exact there;
    the double rounding this may add is far below what is measured)."""
    b, P = z.shape
    total = None
    for c in range(-(-b // ARS_CHUNK)):
        k0, k1 = c * ARS_CHUNK, min(b, (c + 1) * ARS_CHUNK)
        zc, dc = np.zeros((ARS_CHUNK, P)), np.zeros(ARS_CHUNK)
        zc[: k1 - k0], dc[: k1 - k0] = z[k0:k1], d32[k0:k1]                 # past the end: coefficient 0, acc unchanged
        zc, dc = zc.reshape(4, ARS_THREADS, P), dc.reshape(4, ARS_THREADS, 1)
        acc = np.zeros((ARS_THREADS, P), np.float32)
        for k in range(4):
            acc = (dc[k] * zc[k] + acc.astype(np.float64)).astype(np.float32)
        s = ARS_THREADS // 2
        while s:
            acc[:s] = acc[:s] + acc[s:2 * s]
            s >>= 1
        total = acc[0].copy() if total is None else total + acc[0]
    return total


# ---- the update given G and sigma_R -----------------------------------------------------------------------------------------
def step_size(learning_rate, b, sr):
    return np.float32(learning_rate / (float(b) * sr)) if sr > 0.0 else np.float32(0.0)


def update(mu, G, sr, learning_rate, b):
    return (f32(mu) + step_size(learning_rate, b, sr) * f32(G)).astype(np.float32)


class ArsNP:
    """The whole strategy on the host (the float32 sum in the device's order): what the learning test runs."""

    def __init__(self, P, init_sigma, sigma_decay, learning_rate, offspring_num, elite_num=None, seed=0):
        self.P, self.n, self.seed, self.lr = P, offspring_num, seed, learning_rate
        self.b = max(1, offspring_num // 4) if elite_num is None else elite_num
        self.curr_sigma, self.sigma_decay = init_sigma, sigma_decay
        self.mu = np.zeros(P, np.float32)
        self.gen = 0
        self.last_sigma_r = None

    def theta(self):
        return population(self.mu, self.curr_sigma, self.seed, self.gen, 0, self.n)

    def evaluate(self, fitness):
        sel = select(fitness, self.b)
        _, d32 = differences(fitness, sel)
        G = emulate_device_sum(d32, selected_noise(sel, self.seed, self.gen, self.P))
        self.last_sigma_r = sigma_r(fitness, sel)
        self.mu = update(self.mu, G, self.last_sigma_r, self.lr, self.b)
        self.curr_sigma *= self.sigma_decay
        self.gen += 1
        return float(np.max(fitness))
