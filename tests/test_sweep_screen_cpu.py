"""The FP32 screen of the bound pass (option "sweep_screen", kernel_build.hip: THE SCREEN), emulated in numpy: the margin
delta = 2^-24 (d + 8) SC (max |y'| + max |x'|)^2 covers the distance between the screen's u32 and the FP64 test's u for every
pair, a block the screen certifies is one the FP64 test skips, and the screen certifies nearly all of those.

The emulation follows the kernel operation by operation: FP32 images of the centred scaled coordinates, the matrix
instruction as a k-ordered fmaf chain (fl32 of the exact product plus the accumulator, per k), fl32 of the FP64 sum of the two
norms, one last fmaf; blocks of 16 training rows x 32 candidates, one delta per 128 rows x 64 candidates (a workgroup's rows,
a wave's candidates), thresholds rounded inwards to FP32."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

F32 = np.float32
SCALE = {0: 0.5, 2: 3.0, 3: 5.0}        # corr_scale of RBF, Matern-3/2, Matern-5/2
SHAPES = ((257, 16, 2048), (129, 3, 1024), (257, 5, 2048), (129, 21, 1024), (257, 32, 1024), (1000, 16, 2048))


def _fmaf(a, b, c):
    """fl32(a * b + c) for FP32 arrays: the product of two FP32 numbers is exact in FP64, and the FP64 sum rounded to FP32
    is the correctly rounded FP32 result except in double-rounding ties, which the margin does not depend on."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F32)


def _model(seed, N, d, tiny):
    from oracle import gpry_oracle as orc
    from test_sweep_mean_bound_gpu import _short_model
    rng = np.random.default_rng(seed)
    kid = int(rng.choice([0, 2, 3]))
    m, bounds, X = _short_model(rng, orc, d, kid, N)
    ls = np.exp(m.theta[1:])
    if tiny:
        ls = np.full(d, 1e-3)       # every length scale at 1e-3 of the box
    return rng, kid, bounds, X, ls


def _pool(rng, bounds, X, ls, M):
    lo, hi = bounds[:, 0], bounds[:, 1]
    Xc = rng.uniform(lo, hi, (M, len(lo)))
    k = M // 10         # a tenth on and around training rows
    idx = rng.integers(0, len(X), k)
    Xc[:k] = X[idx] + rng.normal(0, 1, (k, len(lo))) * ls * (hi - lo) * rng.choice([0.0, 0.5, 3.0, 10.0], (k, 1))
    return Xc


def _screen(kid, bounds, X, ls, Xc):
    """u of the FP64 test, the screen's u32 and delta per pair (rows padded with zero rows to whole workgroups)."""
    sc = SCALE[kid]
    lo, hi = bounds[:, 0], bounds[:, 1]
    d = X.shape[1]
    Xn = (X - lo) / (hi - lo)
    c = Xn.mean(0)
    Y = (Xn - c) / ls
    Y = np.concatenate([Y, np.zeros((-len(Y) % 128, d))])
    Cn = ((Xc - lo) / (hi - lo) - c) / ls
    yn, xn = (Y * Y).sum(1) * sc, (Cn * Cn).sum(1) * sc
    u64 = -2.0 * sc * (Y @ Cn.T) + (xn[None, :] + yn[:, None])
    Yf, Cf = Y.astype(F32), Cn.astype(F32)
    acc = np.zeros((len(Y), len(Cn)), F32)
    for k in range(d):
        acc = _fmaf(Yf[:, k][:, None], Cf[:, k][None, :], acc)
    s32 = (xn[None, :] + yn[:, None]).astype(F32)
    u32 = _fmaf(np.full_like(acc, F32(-2.0 * sc)), acc, s32).astype(np.float64)
    ny, nx = np.sqrt(yn), np.sqrt(xn)       # (the norms carry the factor SC, as in the kernel)
    delta = 2.0 ** -24 * (d + 8) * (ny[:, None] + nx[None, :]) ** 2
    return u64, u32, delta, yn, xn


def _blocks(a, f, rows, cols):
    n, m = a.shape
    return f(f(a.reshape(n // rows, rows, m // cols, cols), axis=3), axis=1)


def _inwards(lo, hi):
    """[lo, hi] rounded inwards to FP32, elementwise."""
    lo32, hi32 = lo.astype(F32), hi.astype(F32)
    lo32 = np.where(lo32.astype(np.float64) < lo, np.nextafter(lo32, F32(np.inf)), lo32)
    hi32 = np.where(hi32.astype(np.float64) > hi, np.nextafter(hi32, F32(-np.inf)), hi32)
    return lo32.astype(np.float64), hi32.astype(np.float64)


@pytest.mark.parametrize("case", range(len(SHAPES) + 1))
def test_margin_covers_the_screen_and_certified_blocks_are_skipped_blocks(case):
    tiny = case == len(SHAPES)
    N, d, M = SHAPES[0] if tiny else SHAPES[case]
    rng, kid, bounds, X, ls = _model(100 + case, N, d, tiny)
    Xc = _pool(rng, bounds, X, ls, M)
    u64, u32, delta, yn, xn = _screen(kid, bounds, X, ls, Xc)
    sc = SCALE[kid]
    uhi = 1e6 if kid == 0 else 1e12
    worst = float((np.abs(u32 - u64) / delta).max())
    print(f"N={N} d={d} M={M} kid={kid} tiny={tiny}: worst |u32 - u64| / delta = {worst:.3g}")
    assert np.all(np.abs(u32 - u64) <= delta)                                       # assert 1
    # the kernel's delta: one per 128 rows x 64 candidates, from the largest norms in each
    ymax = np.sqrt(yn.reshape(-1, 128).max(1))
    xmax = np.sqrt(xn.reshape(-1, 64).max(1))
    dw = 2.0 ** -24 * (d + 8) * (ymax[:, None] + xmax[None, :]) ** 2
    assert np.all(_blocks(delta, np.max, 128, 64) <= dw)
    dw = np.repeat(np.repeat(dw, 8, axis=0), 2, axis=1)                             # per block of 16 x 32
    mn, mx = _blocks(u32, np.min, 16, 32), _blocks(u32, np.max, 16, 32)
    for mult in (100.0, 500.0, 2500.0, 10000.0):
        ubnd = mult * sc / 5.0
        skip64 = _blocks((u64 >= ubnd) & (u64 <= uhi), np.min, 16, 32).astype(bool)
        lo32, hi32 = _inwards(ubnd + dw, uhi - dw)
        cert = (mn >= lo32) & (mx <= hi32)
        n_skip, n_cert = int(skip64.sum()), int(cert.sum())
        print(f"  ubnd = {ubnd:g}: {skip64.size} blocks, FP64 test skips {n_skip}, screen certifies {n_cert}")
        assert not np.any(cert & ~skip64)                                           # assert 2
        if n_skip >= 100:
            assert n_cert >= 0.95 * n_skip                                          # assert 3

