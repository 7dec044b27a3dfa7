"""Host build of BipedalWalkerHardcore-v3 (tests/walker_hardcore_host.cpp: csrc/ses_walker_hardcore_env.h compiled for the CPU) --
TEST INFRASTRUCTURE.

Compiled on first use into tests/_build/ under a file lock, with the floating-point flags of oracle/Makefile; HardcoreSim drives one env
step by step like c_oracle.WalkerSim, rollout() plays whole populations with the oracle's policy (c_oracle.policy_forward)."""
import ctypes
import fcntl
import os
import re
import subprocess

import numpy as np

from oracle import c_oracle as co

NAME = "BipedalWalkerHardcore-v3"
S, A, INIT_W = 24, 4, 4
STEP = np.float32(14.0) / np.float32(30.0)
TERRAIN_HEIGHT = np.float32(400.0 / 30.0 / 4.0)
COLS = 199
NSLOT = 8
KIND_GROUND, KIND_STUMP, KIND_PIT_FLOOR, KIND_TREAD = 0, 1, 2, 3
_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_HERE)
_CSRC = os.path.join(_ROOT, "simple-es_amd", "csrc")
_SO = os.path.join(_HERE, "_build", "libwalker_hardcore_host.so")
_lib = None


def _fpflags():
    text = open(os.path.join(_ROOT, "oracle", "Makefile")).read()
    return re.search(r"^FPFLAGS\s*:=\s*(.*)$", text, re.M).group(1).split()


def build():
    srcs = [os.path.join(_HERE, "walker_hardcore_host.cpp"), os.path.join(_ROOT, "oracle", "ses_oracle_math.h")]
    srcs += [os.path.join(_CSRC, f) for f in ("ses_b2.h", "ses_b2_toi.h", "ses_b2_shapes.h", "ses_walker_env.h", "ses_walker_hardcore_env.h")]
    newest = max(os.path.getmtime(f) for f in srcs)

    def stale():
        return not os.path.exists(_SO) or os.path.getmtime(_SO) < newest

    if stale():
        os.makedirs(os.path.dirname(_SO), exist_ok=True)
        with open(os.path.join(os.path.dirname(_SO), ".build.lock"), "w") as lock:      # one builder at a time
            fcntl.flock(lock, fcntl.LOCK_EX)
            try:
                if stale():
                    tmp = _SO + ".%d.tmp" % os.getpid()
                    subprocess.check_call([os.environ.get("CXX", "g++")] + _fpflags() +
                                          ["-std=c++17", "-fno-exceptions", "-fno-rtti", "-I", _CSRC, "-I", os.path.join(_ROOT, "oracle"),
                                           "-shared", srcs[0], "-o", tmp, "-lm"])
                    os.replace(tmp, _SO)
            finally:
                fcntl.flock(lock, fcntl.LOCK_UN)
    return _SO


def lib():
    global _lib
    if _lib is None:
        _lib = ctypes.CDLL(build())
        _lib.bwh_step.restype = ctypes.c_float
        _lib.bwh_row_raycast.restype = ctypes.c_float
        _lib.bwh_row_raycast.argtypes = [ctypes.c_void_p] + [ctypes.c_float] * 4
        _lib.bwh_row_index_of.argtypes = [ctypes.c_void_p, ctypes.c_float]
        _lib.bw_index_of.argtypes = [ctypes.c_void_p, ctypes.c_float]
        _lib.bwh_shift.argtypes = [ctypes.c_void_p, ctypes.c_float, ctypes.c_float]
        _lib.bw_shift.argtypes = [ctypes.c_void_p, ctypes.c_float, ctypes.c_float]
        _lib.bwh_row_generate.argtypes = [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p]
        _lib.bw_terrain_heights.argtypes = [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p]
    return _lib


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def init_row(key, force=0.5):
    """an init row [force uniform, terrain key word 0, word 1, pad] whose key words are (key, 0) as bit patterns"""
    row = np.zeros(4, np.float32)
    row[0] = force
    row.view(np.uint32)[1] = key
    return row


# ---- terrain rows -----------------------------------------------------------------------------------------------------------------
def row_generate(key0, key1=0):
    """(row float32[548], kind uint8[199]) of the terrain of one key"""
    row, kind = np.zeros(lib().bwh_row_floats(), np.float32), np.zeros(COLS, np.uint8)
    lib().bwh_row_generate(int(key0), int(key1), _p(row), _p(kind))
    return row, kind


def row_from_spans(yl, yr):
    row = np.zeros(lib().bwh_row_floats(), np.float32)
    yl, yr = np.ascontiguousarray(yl, np.float32), np.ascontiguousarray(yr, np.float32)
    assert yl.shape == yr.shape == (COLS,)
    lib().bwh_row_from_spans(_p(yl), _p(yr), _p(row))
    return row


def row_edges(row):
    """float32[n, 4] = x1, y1, x2, y2 in polyline order"""
    edges = np.zeros((400, 4), np.float32)
    n = lib().bwh_row_edges(_p(row), _p(edges))
    return edges[:n].copy()


def row_index_of(row, x):
    return lib().bwh_row_index_of(_p(row), float(x))


def row_raycast(row, p1, p2):
    return np.float32(lib().bwh_row_raycast(_p(row), float(p1[0]), float(p1[1]), float(p2[0]), float(p2[1])))


def walker_terrain(key0, key1=0):
    """BipedalWalker-v3's 200 heights, edges [199, 4] for one key, by this build's Philox"""
    ty, edges = np.zeros(200, np.float32), np.zeros((199, 4), np.float32)
    lib().bw_terrain_heights(int(key0), int(key1), _p(ty))
    assert lib().bw_edges(_p(ty), _p(edges)) == 199
    return ty, edges


def walker_index_of(ty, x):
    return lib().bw_index_of(_p(ty), float(x))


def vertices(bodies):
    """world vertices of the hull and the four leg polygons of bodies [5, 6]: a list of five float32[n_b, 2]"""
    b = np.ascontiguousarray(bodies, np.float32).reshape(5, 6)
    verts, counts = np.zeros((5, 6, 2), np.float32), np.zeros(5, np.int32)
    lib().bwh_vertices(_p(b), _p(verts), _p(counts))
    return [verts[i, :counts[i]].copy() for i in range(5)]


def shift_walker_sim(sim, dx, dy):
    """c_oracle.WalkerSim (BipedalWalker-v3): every body moved by (dx, dy)"""
    lib().bw_shift(sim._buf, float(dx), float(dy))


class HardcoreSim:
    """one BipedalWalkerHardcore-v3 env driven step by step"""

    def __init__(self):
        self._buf = ctypes.create_string_buffer(lib().bwh_state_size())

    def reset(self, u4):
        u4 = np.ascontiguousarray(u4, np.float32).reshape(4)
        obs = np.empty(S, np.float32)
        lib().bwh_reset(self._buf, _p(u4), _p(obs))
        return obs

    def step(self, action):
        a = np.ascontiguousarray(np.asarray(action, np.float32).reshape(4))
        obs = np.empty(S, np.float32)
        done = ctypes.c_int32(0)
        r = lib().bwh_step(self._buf, _p(a), _p(obs), ctypes.byref(done))
        return obs, np.float32(r), bool(done.value)

    def obs(self):
        obs = np.empty(S, np.float32)
        lib().bwh_obs(self._buf, _p(obs))
        return obs

    def shift(self, dx, dy):
        lib().bwh_shift(self._buf, float(dx), float(dy))

    def blob(self):
        """uint8[blob bytes]: the device's state blob of this env (env struct, then terrain row)"""
        return np.frombuffer(self._buf.raw[:lib().bwh_blob_size()], np.uint8).copy()

    def terrain(self):
        row, kind = np.zeros(lib().bwh_row_floats(), np.float32), np.zeros(COLS, np.uint8)
        lib().bwh_state_row(self._buf, _p(row), _p(kind))
        return row, kind

    def manifolds(self):
        """(flags int32[4, 8], edges int32[4, 8]) of the leg manifolds: -1 not touching, 0 on a ground edge, 1 on an obstacle edge"""
        flags, edges = np.zeros((4, NSLOT), np.int32), np.zeros((4, NSLOT), np.int32)
        lib().bwh_manifold_flags(self._buf, _p(flags), _p(edges))
        return flags, edges

    def on_obstacle(self):
        return bool((self.manifolds()[0] == 1).any())

    def debug(self):
        bodies, ints = np.empty((5, 6), np.float32), np.zeros(5, np.int32)
        lib().bwh_debug(self._buf, _p(bodies), _p(ints))
        return {"bodies": bodies, "game_over": bool(ints[0]), "leg_contact": ints[1:5].astype(bool)}

    def leg_vertices(self):
        """float32[16, 2]: the world vertices of the four leg polygons"""
        return np.concatenate(vertices(self.debug()["bodies"])[1:])


def rollout(theta, init, E, max_step, *, gru=False, touched=None):
    """Population rollout as the fused kernels play it.  init: [E, 4] or [N, E, 4].  Returns (fitness f32[N], ep_return f64[N, E],
    ep_steps i32[N, E]).  touched (bool[N, E], optional) is set where a leg manifold lay on an obstacle edge after some step."""
    theta = np.atleast_2d(np.ascontiguousarray(theta, np.float32))
    init = np.ascontiguousarray(init, np.float32)
    N = theta.shape[0]
    ep_ret, ep_steps, fit = np.empty((N, E), np.float64), np.empty((N, E), np.int32), np.empty(N, np.float32)
    sim = HardcoreSim()
    for i in range(N):
        for e in range(E):
            obs = sim.reset(init[i, e] if init.ndim == 3 else init[e])
            h = np.zeros((1, co.HIDDEN), np.float32) if gru else None
            ret, steps, done, hit = 0.0, 0, False, False
            while not done and steps < max_step:
                _, _, act, h = co.policy_forward(S, A, False, gru, theta[i:i + 1], obs[None], h)
                obs, r, done = sim.step(act[0])
                ret += float(r)
                steps += 1
                if touched is not None and not hit:
                    hit = sim.on_obstacle()
            ep_ret[i, e], ep_steps[i, e] = ret, steps
            if touched is not None:
                touched[i, e] = hit
        total = 0.0
        for e in range(E):
            total += float(ep_ret[i, e])
        fit[i] = np.float32(total / float(E))
    return fit, ep_ret, ep_steps
