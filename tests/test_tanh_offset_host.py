"""tanh_offset_scaled (csrc/ses_math.h) against tanh_index_scaled, on the host: offset == 16 * index and the same fraction, bit for bit.

The fused CartPole loops find a tanh entry by the bit pattern of floor(t) * 2^-145, a subnormal whose bits are 16 * floor(t), where
the other kernels convert t to an integer and shift it.  Both host fallbacks are the expressions the device evaluates (the
fraction is t - floor(t) where the device has v_fract_f32), compiled with the compiler's default flags: no -ffast-math and nothing
that flushes subnormals to zero -- with either, the offset of every entry but the first would read 0 and this test fails."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "simple-es_amd", "csrc")

HARNESS = r'''
#include "ses_math.h"
extern "C" {
void v_index(const float* x, int* idx, float* u, int n) { for (int i = 0; i < n; i++) idx[i] = ses::tanh_index_scaled(x[i], u[i]); }
void v_offset(const float* x, unsigned* off, float* u, int n) { for (int i = 0; i < n; i++) off[i] = ses::tanh_offset_scaled(x[i], u[i]); }
}
'''


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    d = tmp_path_factory.mktemp("tanh_offset")
    (d / "h.cpp").write_text(HARNESS)
    subprocess.check_call(["g++", "-std=c++20", "-shared", "-fPIC", "-I", CSRC, str(d / "h.cpp"), "-o", str(d / "h.so")])
    return ctypes.CDLL(str(d / "h.so"))


def inputs():
    ks = np.arange(0, 321, dtype=np.float32)
    near = [ks]
    lo, hi = ks.copy(), ks.copy()
    for _ in range(4):
        lo, hi = np.nextafter(lo, np.float32(-np.inf)), np.nextafter(hi, np.float32(np.inf))
        near += [lo.copy(), hi.copy()]
    tiny = np.finfo(np.float32)
    special = np.array([0.0, -0.0, tiny.smallest_subnormal, tiny.smallest_normal, 319.99997, 320.0, 1e30, np.inf, -np.inf, np.nan],
                       np.float32)
    pos = np.concatenate(near + [special])
    rnd = np.random.RandomState(0).randint(0, 1 << 32, 1 << 22, dtype=np.uint64).astype(np.uint32)
    # A SIGNALLING NaN among the patterns is made quiet (same sign and payload, quiet bit set): the reference is undefined for it --
    # libm's fminf returns NaN for a signalling operand and tanh_index_scaled then converts NaN to an integer -- and no kernel can
    # meet one: the argument is the result of an fma chain, and an IEEE operation never returns a signalling NaN.
    snan = ((rnd & 0x7F800000) == 0x7F800000) & ((rnd & 0x007FFFFF) != 0) & ((rnd & 0x00400000) == 0)
    rnd = np.where(snan, rnd | 0x00400000, rnd).astype(np.uint32).view(np.float32)
    return np.ascontiguousarray(np.concatenate([pos, -pos, rnd]))


def test_offset_is_sixteen_times_the_index_and_the_fraction_is_the_same(lib):
    x = inputs()
    n = x.size
    idx, off = np.empty(n, np.int32), np.empty(n, np.uint32)
    u_idx, u_off = np.empty(n, np.float32), np.empty(n, np.float32)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    lib.v_index(p(x), p(idx), p(u_idx), ctypes.c_int(n))
    lib.v_offset(p(x), p(off), p(u_off), ctypes.c_int(n))
    assert idx.min() == 0 and idx.max() == 319, (idx.min(), idx.max())           # every entry of the table, and none past it
    bad = off != 16 * idx.astype(np.uint32)
    assert not bad.any(), (int(bad.sum()), x[bad][:8], off[bad][:8], idx[bad][:8])
    bad = u_idx.view(np.uint32) != u_off.view(np.uint32)
    assert not bad.any(), (int(bad.sum()), x[bad][:8])
    assert len(np.unique(idx)) == 320
