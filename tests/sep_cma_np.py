"""numpy restatement of the sep_cma_es strategy (include/ses.h: ses_perturb_sepcma, ses_sepcma_generation) and the float64
reference of its two sums with the bound the device is held to.  Imports no product code; the normals are the C oracle's Philox
normals, bit-identical to the device's.

Constants (double, from (n, P, mu); mu = the number of selected rows, default n // 2)
    w_k ~ ln(mu + 0.5) - ln(k + 1), k < mu, normalised to sum 1; the kernel reads them as the float32 table weights[mu]
    mueff = 1 / sum w^2 (of the double weights);  c_sigma = (mueff + 2) / (P + mueff + 5)
    d_sigma = 1 + 2 max(0, sqrt((mueff - 1) / (P + 1)) - 1) + c_sigma;  c_c = (4 + mueff / P) / (P + 4 + 2 mueff / P)
    c_1 = min(1, (P + 2) / 3 * 2 / ((P + 1.3)^2 + mueff))
    c_mu = min(1 - c_1, (P + 2) / 3 * 2 (mueff - 2 + 1 / mueff) / ((P + 2)^2 + mueff));  chi = sqrt(P) (1 - 1 / (4 P) + 1 / (21 P^2))

Population (bit-exact: one float32 rounding per operation, no fma, sqrt correctly rounded)
    theta[i][p] = fl(mu[p] + fl(fl(fl(float32(sigma) * step) * sqrt(C[p])) * z_ip)),  z_i = noise(seed, gen, row = i)

Sums, in float64 here, with w_i = (double)weights[rank_i] for rank_i < mu and 0 otherwise (ties: higher index first):
    Sz[p] = sum_i w_i z_ip,  Szz[p] = sum_i w_i z_ip^2

The bound (sepcma_tolerance), in the form of pgpe_np.pgpe_tolerance:
    tol[p] = gamma_K * sum_i |w_i t_ip|,   gamma_K = K u / (1 - K u), u = 2^-24,  t = z for Sz and z^2 for Szz
(no weight term: the float32 table IS the definition of the weights, device and float64 reference read the same numbers).  K
counts the float32 roundings one term w_i t_ip can meet on its way through k_sepcma_sums_partial and k_sepcma_update
(csrc/ses_sepcma.hip):
    4        the thread's fma chain: thread c of 256 takes the rows c, c + 256, c + 512, c + 768 of its 1024-row chunk, a term
             enters at one fma and is rounded by it and by every later one (a skipped row rounds nothing): CHUNK / THREADS = 4;
    8        the LDS tree over the 256 threads: log2(256) additions;
    chunks   the ordered sum of the chunk partials (chunks - 1 additions; one is spare, as in pgpe_rounding_count);
    +1       for Szz only: fl(z z) rounds t itself once.
K = 12 + chunks for Sz, 13 + chunks for Szz (chunks = ceil(n / 1024)): 13 ... 22 at the sizes the tests use.

norm2 = sum_p (double)p_sigma'[p]^2, in the device's order (norm2_device_order): thread c of 1024 adds the squares of p = c,
c + 1024, ... in ascending order to 0.0, then x[c] += x[c + s] for s = 512 ... 1.  The squares are exact in double, so numpy
float64 reproduces the device bit for bit.
"""
import math

import numpy as np

from oracle import c_oracle as co
from oracle import strategies_np as snp

CHUNK = 1024               # rows per workgroup of the sums (csrc/ses_sepcma.hip SEPCMA_CHUNK)
THREADS = 256
UPDATE_THREADS = 1024      # SEPCMA_UPDATE_THREADS
F32_U = 2.0 ** -24
DEFAULTS = dict(scale_limits=(0.01, 100.0), step_limits=(1e-6, 1e6))


def f32(x):
    return np.asarray(x, dtype=np.float32)


# ---- constants ------------------------------------------------------------------------------------------------------------
def constants(n, P, mu=None):
    """(dict of the doubles + mu, float32 weights[mu])"""
    mu = n // 2 if mu is None else int(mu)
    w = math.log(mu + 0.5) - np.log(np.arange(1, mu + 1, dtype=np.float64))
    w = w / w.sum()
    mueff = 1.0 / float((w * w).sum())
    c_sigma = (mueff + 2.0) / (P + mueff + 5.0)
    d_sigma = 1.0 + 2.0 * max(0.0, math.sqrt((mueff - 1.0) / (P + 1.0)) - 1.0) + c_sigma
    c_c = (4.0 + mueff / P) / (P + 4.0 + 2.0 * mueff / P)
    c_1 = min(1.0, (P + 2.0) / 3.0 * 2.0 / ((P + 1.3) ** 2 + mueff))
    c_mu = min(1.0 - c_1, (P + 2.0) / 3.0 * 2.0 * (mueff - 2.0 + 1.0 / mueff) / ((P + 2.0) ** 2 + mueff))
    chi = math.sqrt(P) * (1.0 - 1.0 / (4.0 * P) + 1.0 / (21.0 * P * P))
    return dict(mu=mu, mueff=mueff, c_sigma=c_sigma, d_sigma=d_sigma, c_c=c_c, c_1=c_1, c_mu=c_mu, chi=chi), w.astype(np.float32)


def hsig_scale(c, t):
    """1 / sqrt(1 - (1 - c_sigma)^(2 t)) of update t (from 1), as the host forms it per generation"""
    return 1.0 / math.sqrt(1.0 - (1.0 - c["c_sigma"]) ** (2.0 * float(t)))


def hsig_threshold(c, P):
    return (1.4 + 2.0 / (P + 1.0)) * c["chi"]


# ---- population -----------------------------------------------------------------------------------------------------------
def population(mu, C, step, sigma, seed, gen, first_row=0, n_rows=None, n=None):
    """rows [first_row, first_row + n_rows) of the population, float32, bit for bit what the device writes"""
    mu, C = f32(mu), f32(C)
    if n_rows is None:
        n_rows = n - first_row
    z = co.noise(seed, gen, first_row, n_rows, mu.shape[0])
    s0 = np.float32(sigma) * np.float32(step)             # float32 * float32 -> one rounding
    sd = s0 * np.sqrt(C)
    return np.ascontiguousarray(mu[None, :] + sd[None, :] * z)


# ---- weights ----------------------------------------------------------------------------------------------------------------
def row_weights(fitness, weights):
    """float64[n]: (double)weights[rank_i] for rank_i < mu, else 0 (ties: higher index first)"""
    rank = snp.stable_rank(np.asarray(fitness))
    w = np.zeros(len(rank))
    sel = rank < len(weights)
    w[sel] = weights.astype(np.float64)[rank[sel]]
    return w


# ---- float64 sums and their bound -------------------------------------------------------------------------------------------
def chunk_sums_f64(w, seed, gen, P, noise=None):
    """Per chunk of CHUNK rows: dict of float64 [chunks, P] arrays Sz = sum w z, Az = sum |w z|, Szz = sum w z^2 (= sum |w z^2|:
    the weights are not negative)."""
    noise = co.noise if noise is None else noise
    n = len(w)
    out = {k: [] for k in ("Sz", "Az", "Szz")}
    for c in range(-(-n // CHUNK)):
        i0, i1 = c * CHUNK, min(n, (c + 1) * CHUNK)
        z = noise(seed, gen, i0, i1 - i0, P).astype(np.float64)
        out["Sz"].append(w[i0:i1] @ z)
        out["Az"].append(np.abs(w[i0:i1]) @ np.abs(z))
        out["Szz"].append(w[i0:i1] @ (z * z))
    return {k: np.stack(v) for k, v in out.items()}


def rounding_count(n, which):
    chunks = -(-n // CHUNK)
    K = CHUNK // THREADS + int(np.log2(THREADS)) + chunks
    return K + (1 if which == "zz" else 0)


def sepcma_tolerance(n, which, term_abs):
    """tol[P] for |S_device - S64|; which = "z" or "zz"; term_abs = sum_i |w_i t_ip| (float64)"""
    K = rounding_count(n, which)
    return K * F32_U / (1.0 - K * F32_U) * term_abs


def sums_f64(fitness, weights, seed, gen, P):
    """(Sz64, Szz64, tol_z, tol_zz): the float64 sums of a fitness vector and the device's allowance around each"""
    n = len(fitness)
    cs = chunk_sums_f64(row_weights(fitness, weights), seed, gen, P)
    return (cs["Sz"].sum(0), cs["Szz"].sum(0), sepcma_tolerance(n, "z", cs["Az"].sum(0)), sepcma_tolerance(n, "zz", cs["Szz"].sum(0)))


# ---- the device's summation order in float32 (host emulation) ------------------------------------------------------------------
def emulate_device_sums(w, seed, gen, P):
    """float32 (Sz, Szz) in k_sepcma_sums_partial's and k_sepcma_update's order.  The fmas are emulated in float64 (the products
    are exact there; the double rounding this may add is far below what is measured).  A skipped row is a row of weight 0: the
    fma leaves the accumulator as it is."""
    n = len(w)
    wf = w.astype(np.float32).astype(np.float64)
    tot_z = tot_zz = None
    for c in range(-(-n // CHUNK)):
        i0, i1 = c * CHUNK, min(n, (c + 1) * CHUNK)
        z = np.zeros((CHUNK, P), np.float32)
        z[: i1 - i0] = co.noise(seed, gen, i0, i1 - i0, P)
        zz = (z * z).astype(np.float64)                                  # fl(z z): one float32 rounding
        z = z.astype(np.float64)
        wc = np.zeros(CHUNK)
        wc[: i1 - i0] = wf[i0:i1]
        z, zz, wc = z.reshape(4, THREADS, P), zz.reshape(4, THREADS, P), wc.reshape(4, THREADS, 1)
        acc_z = np.zeros((THREADS, P), np.float32)
        acc_zz = np.zeros((THREADS, P), np.float32)
        for k in range(4):
            acc_z = (wc[k] * z[k] + acc_z.astype(np.float64)).astype(np.float32)
            acc_zz = (wc[k] * zz[k] + acc_zz.astype(np.float64)).astype(np.float32)
        s = THREADS // 2
        while s:
            acc_z[:s] = acc_z[:s] + acc_z[s:2 * s]
            acc_zz[:s] = acc_zz[:s] + acc_zz[s:2 * s]
            s >>= 1
        tot_z = acc_z[0].copy() if tot_z is None else tot_z + acc_z[0]
        tot_zz = acc_zz[0].copy() if tot_zz is None else tot_zz + acc_zz[0]
    return tot_z, tot_zz


# ---- the update given the two sums ----------------------------------------------------------------------------------------------
def path_sigma(ps, Sz, c):
    """p_sigma' = fl(fl(a_s p_sigma) + fl(b_s Sz))"""
    a_s = np.float32(1.0 - c["c_sigma"])
    b_s = np.float32(math.sqrt(c["c_sigma"] * (2.0 - c["c_sigma"]) * c["mueff"]))
    return a_s * f32(ps) + b_s * f32(Sz)


def norm2_device_order(ps_new):
    """sum_p (double)ps_new[p]^2 in k_sepcma_update's order, float64, bit for bit"""
    sq = f32(ps_new).astype(np.float64) ** 2
    P = sq.shape[0]
    rounds = -(-P // UPDATE_THREADS)
    pad = np.zeros(rounds * UPDATE_THREADS)
    pad[:P] = sq
    acc = np.zeros(UPDATE_THREADS)
    for r in pad.reshape(rounds, UPDATE_THREADS):
        acc = acc + r
    s = UPDATE_THREADS // 2
    while s:
        acc[:s] = acc[:s] + acc[s:2 * s]
        s >>= 1
    return float(acc[0])


def scalar_path(norm2, step, c, P, hs_scale, step_limits=(1e-6, 1e6)):
    """(h, step') from norm2, in double as the one thread of k_sepcma_update computes them; step' rounded and clamped in float32"""
    nrm = math.sqrt(norm2)
    h = nrm * hs_scale < hsig_threshold(c, P)
    e = (c["c_sigma"] / c["d_sigma"]) * (nrm / c["chi"] - 1.0)
    capped = e > 1.0
    if capped:
        e = 1.0
    sn = np.float32(float(np.float32(step)) * math.exp(e))
    out = np.minimum(np.maximum(sn, np.float32(step_limits[0])), np.float32(step_limits[1]))
    return bool(h), np.float32(out), dict(nrm=nrm, exponent=e, capped=capped, unclamped=sn)


def update(mu, C, ps, pc, step, Sz, Szz, norm2, sigma, hs_scale, c, scale_limits=(0.01, 100.0), step_limits=(1e-6, 1e6)):
    """((mu, C, p_sigma, p_c, step)', h, info) after the generation whose sums are (Sz, Szz) and whose |p_sigma'|^2 is norm2; one
    numpy float32 operation per device operation.  sigma: the curr_sigma the evaluated population was drawn with."""
    mu, C, ps, pc, Sz, Szz = (f32(x) for x in (mu, C, ps, pc, Sz, Szz))
    P = mu.shape[0]
    ps_new = path_sigma(ps, Sz, c)
    h, step_new, info = scalar_path(norm2, step, c, P, hs_scale, step_limits)
    sC = np.sqrt(C)
    y = sC * Sz
    a_c = np.float32(1.0 - c["c_c"])
    hb = np.float32(math.sqrt(c["c_c"] * (2.0 - c["c_c"]) * c["mueff"])) if h else np.float32(0.0)
    pc_new = a_c * pc + hb * y
    sd = (np.float32(sigma) * np.float32(step)) * sC
    mu_new = mu + sd * Sz
    k0 = np.float32(1.0 - c["c_1"] - c["c_mu"] + (0.0 if h else c["c_1"] * c["c_c"] * (2.0 - c["c_c"])))
    c1f, cmuf = np.float32(c["c_1"]), np.float32(c["c_mu"])
    lo, hi = np.float32(scale_limits[0]), np.float32(scale_limits[1])
    raw = (k0 * C + c1f * (pc_new * pc_new)) + cmuf * (C * Szz)
    C_new = np.minimum(np.maximum(raw, lo * lo), hi * hi).astype(np.float32)
    info["C_raw"] = raw
    return (mu_new, C_new, ps_new, pc_new, step_new), h, info


class SepCmaNP:
    """The whole strategy on the host (float32 sums in the device's order): what the learning test runs."""

    def __init__(self, P, init_sigma, sigma_decay, offspring_num, elite_num=None, seed=0, **kw):
        self.P, self.n, self.seed, self.kw = P, offspring_num, seed, {**DEFAULTS, **kw}
        self.c, self.weights = constants(offspring_num, P, elite_num)
        self.curr_sigma, self.sigma_decay = init_sigma, sigma_decay
        self.mu, self.C = np.zeros(P, np.float32), np.ones(P, np.float32)
        self.ps, self.pc = np.zeros(P, np.float32), np.zeros(P, np.float32)
        self.step = np.float32(1.0)
        self.t = 0
        self.gen = 0

    def theta(self):
        return population(self.mu, self.C, self.step, self.curr_sigma, self.seed, self.gen, 0, self.n)

    def evaluate(self, fitness):
        w = row_weights(fitness, self.weights)
        Sz, Szz = emulate_device_sums(w, self.seed, self.gen, self.P)
        self.t += 1
        norm2 = norm2_device_order(path_sigma(self.ps, Sz, self.c))
        (self.mu, self.C, self.ps, self.pc, self.step), self.h, _ = update(
            self.mu, self.C, self.ps, self.pc, self.step, Sz, Szz, norm2, self.curr_sigma, hsig_scale(self.c, self.t), self.c, **self.kw)
        self.curr_sigma *= self.sigma_decay
        self.gen += 1
        return float(np.max(fitness))
