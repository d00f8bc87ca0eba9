"""CPU proof of tests/dense_ref.py, the host reference of tests/test_dense_kernels_gpu.py:
  * its fmaf emulation is glibc's correctly rounded fmaf on random and adversarial triples (ties, near-ties, cancellation, exponent
    gaps, subnormals);
  * defects planted in a host emulation of the kernels fail the same comparison functions the GPU tests apply, so every bound is
    tight enough to matter."""
import ctypes
import ctypes.util

import numpy as np
import pytest

import dense_ref as R

_libm = ctypes.CDLL(ctypes.util.find_library('m') or 'libm.so.6')
_libm.fmaf.argtypes = (ctypes.c_float, ctypes.c_float, ctypes.c_float)
_libm.fmaf.restype = ctypes.c_float


def _glibc_fmaf(a, b, c):
    return np.array([_libm.fmaf(float(x), float(y), float(z)) for x, y, z in zip(a, b, c)], dtype=np.float32)


def _triples(rng, n):
    f = np.float32
    out = []
    # random magnitudes over a wide exponent range, both signs
    e = lambda k: np.exp2(rng.integers(-40, 40, k)).astype(np.float64)
    out.append([(rng.standard_normal(n) * e(n)).astype(f) for _ in range(3)])
    # exact and near ties: a*b = d (1 - 2^-2k) with d an odd multiple of half an ulp of c, so c + a*b sits on or just off a float32
    # midpoint (exactly on it in float64 for k >= 18)
    c = (rng.standard_normal(n) * e(n)).astype(f)
    ulp = np.spacing(np.abs(c)).astype(np.float64)
    d = (2 * rng.integers(0, 8, n) + 1) * ulp / 2 * rng.choice([-1.0, 1.0], n)
    k = rng.integers(8, 21, n).astype(np.float64)
    a = (1 + np.exp2(-k)).astype(f)
    b = (d * (1 - np.exp2(-k))).astype(f)
    out.append([a, b, c])
    # plain ties: a*b exactly half an ulp of c (round half to even decides)
    out.append([np.ones(n, f), (ulp / 2 * rng.choice([-1.0, 1.0], n)).astype(f), c])
    # cancellation: c = -fl(a*b)
    a = (rng.standard_normal(n) * e(n)).astype(f)
    b = (rng.standard_normal(n)).astype(f)
    out.append([a, b, (-(a.astype(np.float64) * b)).astype(f)])
    # exponent gaps: |c| >> |a*b| and |a*b| >> |c|; subnormal results
    out.append([a, b, (rng.standard_normal(n) * np.exp2(60.0)).astype(f)])
    out.append([a, b, (rng.standard_normal(n) * np.exp2(-100.0)).astype(f)])
    out.append([(rng.standard_normal(n) * 2.0 ** -70).astype(f), (rng.standard_normal(n) * 2.0 ** -70).astype(f),
                (rng.standard_normal(n) * 2.0 ** -140).astype(f)])
    return [np.concatenate(t) for t in zip(*out)]


def test_fmaf_matches_glibc():
    rng = np.random.default_rng(0)
    a, b, c = _triples(rng, 15000)
    assert len(a) >= 100000
    got = R.fmaf(a, b, c)
    ref = _glibc_fmaf(a, b, c)
    same = (got.view(np.uint32) == ref.view(np.uint32)) | (np.isnan(got) & np.isnan(ref))
    assert same.all(), (a[~same][:3], b[~same][:3], c[~same][:3], got[~same][:3], ref[~same][:3])
    # the midpoint correction is exercised: a plain double rounding gets some of them wrong
    naive = (a.astype(np.float64) * b + c).astype(np.float32)
    assert (naive.view(np.uint32) != ref.view(np.uint32)).sum() > 100


def test_chain_order_is_the_mfma_k_order():
    assert R.chain_order(16) == [0, 4, 1, 5, 2, 6, 3, 7, 8, 12, 9, 13, 10, 14, 11, 15]


# ------------------------------------------------------------------------------------------------------------- planted defects
def _data(rng, M=64, N=256, K=128, positive=False):
    x = np.abs(rng.standard_normal((M, K))).astype(np.float32)
    w = (rng.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32)
    return x, (np.abs(w) if positive else w)


def _pieces_check(out, x, w, mode):
    """the GPU tests' comparison of a split kernel with its exact piece products (test_gemm_split_pieces_and_bound)"""
    S, A = R.piece_sum(x, w, mode)
    return R.check_bound(out, S, R.gamma(x.shape[1]) * A, mode)


@pytest.mark.parametrize('mode', ['bf16x3', 'f16x3', 'f16fp8x2'])
def test_faithful_emulation_passes(mode):
    rng = np.random.default_rng(1)
    x, w = _data(rng)
    out = R.piece_sum(x, w, mode)[0].astype(np.float32)
    assert _pieces_check(out, x, w, mode) <= 1.0
    ref, bnd = R.dense_bound(x.astype(np.float64), np.zeros_like(x, dtype=np.float64), w, None, mode, x.shape[1])
    assert R.check_bound(out, ref, bnd, mode) <= 1.0


@pytest.mark.parametrize('mode', ['bf16x3', 'f16x3'])
def test_dropping_x_lo_w_hi_on_one_block_fails(mode):
    rng = np.random.default_rng(2)
    x, w = _data(rng)
    bad = R.piece_sum(x, w, mode, drop=(0, slice(48, 64)))[0].astype(np.float32)
    with pytest.raises(AssertionError):
        _pieces_check(bad, x, w, mode)


def test_truncated_lo_piece_fails():
    """lo = trunc(v - hi) instead of rne: with weights whose residuals lose most of a lo ulp to truncation, the bias is coherent over
    K (bf16 pieces: up to 2^-16 of each product, above gamma_128 = 2^-17 of the magnitudes).  With f16 pieces a truncated lo errs
    by at most 2^-22 of a product, below the accumulation's own rounding: no per-element bound resolves it, so bf16 carries the check."""
    rng = np.random.default_rng(3)
    K = 128
    x = np.abs(rng.standard_normal((64, K))).astype(np.float32)
    # w = hi (1 + 2^-9 (1 + 2^-7 - 2^-14)): its residual lies 2^-7 of a lo ulp below the next bf16 value, so rne rounds lo up and
    # truncation drops nearly a whole lo ulp
    hi = np.exp2(rng.integers(-4, 0, (128, K))).astype(np.float64)
    w = (hi * (1 + 2.0 ** -9 * (1 + 2.0 ** -7 - 2.0 ** -14))).astype(np.float32)
    wh, wl = R.split16(w, 'bf16')
    r = w.astype(np.float64) - wh
    bits = r.astype(np.float32).view(np.uint32) & np.uint32(0xffff0000)
    wl_trunc = bits.view(np.float32).astype(np.float64)
    assert (np.abs(wl_trunc) < np.abs(wl)).all()
    xh, xl = R.split16(x, 'bf16')
    bad = (xl @ wh.T + xh @ wl_trunc.T + xh @ wh.T).astype(np.float32)
    with pytest.raises(AssertionError):
        _pieces_check(bad, x, w, 'bf16x3')


def _pointmax_f32(h, w, drop_last_of_tile=None):
    acc = R.fma_chain(h, w)
    if drop_last_of_tile is not None:
        keep = np.ones(h.shape[0], bool)
        keep[drop_last_of_tile - 1::drop_last_of_tile] = False
        acc = acc[keep]
    return acc.max(axis=0)


def test_dropping_the_last_point_of_a_tile_fails():
    rng = np.random.default_rng(4)
    h = np.abs(rng.standard_normal((128, 64))).astype(np.float32)
    w = rng.standard_normal((256, 64)).astype(np.float32)
    with pytest.raises(AssertionError):
        R.check_bitwise(_pointmax_f32(h, w, drop_last_of_tile=64), _pointmax_f32(h, w), 'f32 max')
    # the split modes' bound: the max over points of the exact piece sums
    for mode in ('bf16x3', 'f16x3', 'f16fp8x2'):
        S, A = R.piece_sum(h, w, mode)
        keep = np.ones(128, bool)
        keep[31::32] = False                            # the last point of every wave's 32-point tile
        bad = S[keep].max(axis=0).astype(np.float32)
        with pytest.raises(AssertionError):
            R.check_bound(bad, S.max(axis=0), R.gamma(64) * A.max(axis=0), mode)


def test_swapping_two_k_breaks_bitwise():
    rng = np.random.default_rng(5)
    x, w = _data(rng, M=32, N=64, K=64)
    order = R.chain_order(64)
    swapped = list(order)
    swapped[0], swapped[1] = swapped[1], swapped[0]
    ref = R.fma_chain(x, w)
    assert np.array_equal(R.fma_chain(x, w, order), ref)
    with pytest.raises(AssertionError):
        R.check_bitwise(R.fma_chain(x, w, swapped), ref, 'swapped k')
    # and the plain ascending order is not the kernels' either
    with pytest.raises(AssertionError):
        R.check_bitwise(R.fma_chain(x, w, list(range(64))), ref, 'ascending k')


@pytest.mark.parametrize('shift', [(0, 1), (1, 0), (0, -1)])
def test_wrong_e4m3_scale_exponent_fails(shift):
    rng = np.random.default_rng(6)
    x, w = _data(rng)
    xh, xh8, xl8 = R.mx_pieces(x)
    wh, wh8, wl8 = R.mx_pieces(w, deq_shift=shift)
    bad = (xh @ wh.T + xh8 @ wl8.T + xl8 @ wh8.T).astype(np.float32)
    with pytest.raises(AssertionError):
        _pieces_check(bad, x, w, 'f16fp8x2')
