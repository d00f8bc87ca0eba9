"""cg_ransac_9d and cg_similarity_inliers (csrc/ransac.hip) on the constructed hypotheses of tests/ransac_cases.py, which
tests/test_ransac_cases_cpu.py certifies from the oracle alone.  Every launch goes through the C entry point with sentinel-filled outputs
and two guard rows; every comparison is equality (verdict, count, transform bits, mask bytes) except the transform of the shear
cases, which is within ransac_cases.T_TOL of the oracle's.

Branch of csrc/ransac.hip                                   -> test that pins it
  hypothesis(): pivot search / row swap at columns 0, 1, 2   test_all_orderings_of_the_sample
                relative pivot test (no model)               test_degenerate_samples
                sc[j] > max_scale[j], sc[j] < min_scale[j]   test_scale_bounds_per_axis_and_side (on the bound: kept; one ulp past: -1)
                smin < 0.8 alone / smax > 1.2 alone          test_singular_value_gate_each_side
                det < 0                                      test_reflection
  ransac_9d_kernel: extent, min and max, every wave / lane,  test_extent_gate_single_witness[N] (u - l == max_dims kept, one ulp less: -1,
                    second stride, ragged tail                 no bound: kept)
                    inlier count, same positions             test_inlier_count_single_witness[N] (error == threshold counted, just above not)
                    output rows, H = 1, guard rows           test_output_discipline
  cg_ransac_9d: H = 0, N < 4, threshold < 0 / NaN, null      test_argument_checks
                scale pointers
  similarity_inliers_kernel: N = 1, 255, 256, 257; <=        test_similarity_inliers_mask[N], test_best_mask_sums_to_its_count
  aligning.estimate9DTransform: first maximum, rejected      test_selection_first_maximum_and_all_rejected
                and lower counts in front, none accepted

Measured on an MI355X: no test takes more than 0.2 s, the whole module under 1 s after start-up."""
import ctypes

import numpy as np
import pytest
import torch

import ransac_cases as rc
from oracle import aligning_ref

pytestmark = pytest.mark.gpu
GUARD = 2
COUNT_SENTINEL, T_SENTINEL = -77, 7.25
ZERO16 = np.zeros(16)
D3 = ctypes.c_double * 3


def _d(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _launch(dev, src, dst, ids, thres, min_scale, max_scale, max_dims, N=None):
    """-> status, counts (H), transforms (H,16); sentinels and guard rows checked"""
    from catgrasp_amd import _lib as L
    H = len(ids)
    d_src, d_dst, d_ids = _d(src, dev), _d(dst, dev), _d(np.asarray(ids, dtype=np.int32).reshape(-1, 4), dev)
    counts = torch.full((H + GUARD,), COUNT_SENTINEL, dtype=torch.int32, device=dev)
    tf = torch.full((H + GUARD, 16), T_SENTINEL, dtype=torch.float64, device=dev)
    st = L.lib().cg_ransac_9d(L._p(d_src), L._p(d_dst), len(src) if N is None else N, L._p(d_ids), H, thres,
                              None if min_scale is None else D3(*min_scale), None if max_scale is None else D3(*max_scale),
                              None if max_dims is None else D3(*max_dims), L._p(counts), L._p(tf), L._stream())
    c, t = counts.cpu().numpy(), tf.cpu().numpy()
    assert (c[H:] == COUNT_SENTINEL).all() and (t[H:] == T_SENTINEL).all(), 'guard rows written'
    return st, c[:H], t[:H]


def _run(dev, case):
    st, c, t = _launch(dev, case.src, case.dst, case.ids, case.thres, case.min_scale, case.max_scale, case.max_dims)
    assert st == 0
    for h in range(len(c)):           # every row fully written: [R s | t ; 0 0 0 1] and a count, or 16 zeros and -1
        if c[h] >= 0:
            assert np.array_equal(t[h, 12:], [0, 0, 0, 1]) and not (t[h, :12] == T_SENTINEL).any(), f'{case}[{h}]: {t[h]}'
        else:
            assert c[h] == -1 and np.array_equal(t[h], ZERO16), f'{case}[{h}]: count {c[h]}, row {t[h]}'
    return c, t.reshape(-1, 4, 4)


def _check(dev, case, wrong):
    """verdict, count and transform of every hypothesis of the case against the constructed ones (the oracle's where the case leaves
    them open); mismatches are collected"""
    c, T = _run(dev, case)
    outs = None
    if case.count is None or case.T is None:
        outs = aligning_ref.estimate9DTransform(case.src, case.dst, case.thres, case.ids, case.max_scale, case.min_scale, case.max_dims)[2]
    for h in range(len(c)):
        exp_c = case.count[h] if case.count is not None else (-1 if outs[h] is None else outs[h][0])
        assert (exp_c >= 0) == bool(case.accept[h])
        if c[h] != exp_c:
            wrong.append(f'{case}[{h}]: count {c[h]}, expected {exp_c}')
        elif exp_c >= 0:
            if case.exact:
                if not np.array_equal(T[h], case.T):
                    wrong.append(f'{case}[{h}]: transform off by {np.abs(T[h] - case.T).max():.3e}, expected the constructed bits')
            else:
                gap = float(np.abs(T[h] - outs[h][1]).max())
                print(f'MEASURED {case}: |T_dev - T_oracle| = {gap:.3e}')
                if not gap <= rc.T_TOL:
                    wrong.append(f'{case}[{h}]: transform off the oracle by {gap:.3e} > {rc.T_TOL:.3e}')


def _check_all(dev, cases):
    wrong = []
    for case in cases:
        _check(dev, case, wrong)
    assert not wrong, f'{len(wrong)} mismatches:\n' + '\n'.join(wrong[:40])


def test_scale_bounds_per_axis_and_side(cuda_device):
    _check_all(cuda_device, rc.scale_cases())


def test_singular_value_gate_each_side(cuda_device):
    _check_all(cuda_device, rc.shear_cases())


def test_reflection(cuda_device):
    _check_all(cuda_device, rc.reflection_cases())


def test_all_orderings_of_the_sample(cuda_device):
    _check_all(cuda_device, [rc.orderings()])


def test_degenerate_samples(cuda_device):
    _check_all(cuda_device, rc.degenerate_cases())


@pytest.mark.parametrize('N', rc.NS)
def test_extent_gate_single_witness(cuda_device, N):
    cases = [rc.all_inliers_case(N)]
    for p in rc.positions(N):
        for axis in range(3):
            for end in ('max', 'min'):
                cases += rc.extent_cases(N, p, axis, end)
    _check_all(cuda_device, cases)


@pytest.mark.parametrize('N', rc.NS)
def test_inlier_count_single_witness(cuda_device, N):
    _check_all(cuda_device, [rc.all_inliers_case(N)] + [rc.inlier_case(N, p, above) for p in rc.positions(N) for above in (False, True)])


def test_output_discipline(cuda_device):
    """accepted and rejected rows side by side in one launch, then H = 1 of each: every row fully written (checked by _run / _launch
    for every launch of this module as well), guard rows untouched"""
    src = rc.filler(8); src[4] = [0.25, 0.25, 0.0]
    dst = rc.model(src)
    ids = np.array([[0, 1, 2, 3], [0, 1, 2, 4], [3, 2, 1, 0], [0, 1, 1, 2], [1, 2, 3, 0]], dtype=np.int32)
    exp = np.array([8, -1, 8, -1, 8])
    case = rc.Case('mixed', 'degenerate', src, dst, exp >= 0, count=8, ids=ids, T=rc.mat4(rc.A0, rc.T0))
    c, T = _run(cuda_device, case)
    assert np.array_equal(c, exp) and all(np.array_equal(T[h], case.T) for h in np.flatnonzero(exp >= 0))
    for row in (0, 1):
        one = rc.Case('one', 'degenerate', src, dst, exp[row] >= 0, count=8, ids=ids[row:row + 1], T=case.T)
        c, T = _run(cuda_device, one)
        assert c.tolist() == [exp[row]]


def test_argument_checks(cuda_device):
    """every refusal returns before any launch: the sentinels stay"""
    src, dst = rc.filler(8), rc.model(rc.filler(8))
    ids = np.array([[0, 1, 2, 3]], dtype=np.int32)
    lo, hi = rc.OPEN_MIN, rc.OPEN_MAX

    def untouched(st, c, t, status):
        assert st == status and (c == COUNT_SENTINEL).all() and (t == T_SENTINEL).all()
    untouched(*_launch(cuda_device, src, dst, ids[:0], rc.THRES, lo, hi, None), 0)               # H = 0: OK, nothing written
    for n in (3, 0, -1):
        untouched(*_launch(cuda_device, src, dst, ids, rc.THRES, lo, hi, None, N=n), -1)         # CG_ERR_ARG
    for thres in (-1.0, -5e-324, float('nan')):
        untouched(*_launch(cuda_device, src, dst, ids, thres, lo, hi, None), -1)
    untouched(*_launch(cuda_device, src, dst, ids, rc.THRES, None, hi, None), -1)
    untouched(*_launch(cuda_device, src, dst, ids, rc.THRES, lo, None, None), -1)
    st, c, _ = _launch(cuda_device, src, dst, ids, 0.0, lo, hi, None)                            # threshold 0 is legal: exact inliers only
    assert st == 0 and c.tolist() == [8]


def _mask(dev, src, dst, T, thres, N):
    from catgrasp_amd import _lib as L
    d_src, d_dst, d_T = _d(src, dev), _d(dst, dev), _d(T.reshape(16), dev)
    mask = torch.full((N + 16,), 0xA5, dtype=torch.uint8, device=dev)
    L.check(L.lib().cg_similarity_inliers(L._p(d_src), L._p(d_dst), N, L._p(d_T), thres, L._p(mask), L._stream()), 'cg_similarity_inliers')
    m = mask.cpu().numpy()
    assert (m[N:] == 0xA5).all(), 'guard bytes written'
    return m[:N]


@pytest.mark.parametrize('N', (1, 255, 256, 257))
def test_similarity_inliers_mask(cuda_device, N):
    src, dst, T, exp = rc.mask_case(N)
    assert np.array_equal(_mask(cuda_device, src, dst, T, rc.THRES, N), exp)
    assert len(_mask(cuda_device, src, dst, T, rc.THRES, 0)) == 0            # N = 0: OK, nothing written (guard check inside)


def test_best_mask_sums_to_its_count(cuda_device):
    from catgrasp_amd import aligning
    N = 257
    case = rc.inlier_case(N, 256, False)
    ids = np.array([[0, 1, 1, 2], [0, 1, 2, 3]], dtype=np.int32)
    st, c, t = _launch(cuda_device, case.src, case.dst, ids, rc.THRES, rc.OPEN_MIN, rc.OPEN_MAX, None)
    assert st == 0 and c.tolist() == [-1, 5]
    T, inl = aligning.estimate9DTransform(case.src, case.dst, rc.THRES, ids=ids)
    T_ref, inl_ref, _ = aligning_ref.estimate9DTransform(case.src, case.dst, rc.THRES, ids, rc.OPEN_MAX, rc.OPEN_MIN)
    assert len(inl) == c[1] and np.array_equal(inl, inl_ref) and inl.tolist() == [0, 1, 2, 3, 256]
    assert np.array_equal(T, T_ref) and np.array_equal(T, case.T)
    assert _mask(cuda_device, case.src, case.dst, t[1].reshape(4, 4), rc.THRES, N).sum() == c[1]


def test_selection_first_maximum_and_all_rejected(cuda_device):
    from catgrasp_amd import aligning
    src, dst, m = rc.selection_cloud()
    assert m['a'][2] == m['b'][2] > m['c'][2]
    for order, winner in ((('a', 'b'), 'a'), (('b', 'a'), 'b'), (('bad', 'c', 'a', 'b'), 'a'), (('c', 'bad', 'b', 'c', 'a'), 'b')):
        ids = np.array([m[k][0] for k in order], dtype=np.int32)
        T, inl = aligning.estimate9DTransform(src, dst, rc.THRES, ids=ids)
        T_ref, inl_ref, _ = aligning_ref.estimate9DTransform(src, dst, rc.THRES, ids, rc.OPEN_MAX, rc.OPEN_MIN)
        assert np.array_equal(T, m[winner][1]) and np.array_equal(T, T_ref), order
        assert np.array_equal(inl, inl_ref) and len(inl) == m[winner][2], order
    ids = np.array([m['bad'][0], [4, 4, 5, 6]], dtype=np.int32)
    assert aligning.estimate9DTransform(src, dst, rc.THRES, ids=ids) == (None, None)
    tight = np.nextafter(rc.S3, 0.0)                                    # every hypothesis rejected by a scale bound
    ids = np.array([m[k][0] for k in ('a', 'b', 'c')], dtype=np.int32)
    assert aligning.estimate9DTransform(src, dst, rc.THRES, ids=ids, max_scale=tight) == (None, None)
    assert aligning_ref.estimate9DTransform(src, dst, rc.THRES, ids, tight, rc.OPEN_MIN)[0] is None
