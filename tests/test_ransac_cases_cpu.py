"""The constructed hypotheses of tests/ransac_cases.py are what they claim, from the oracle (oracle/aligning_ref.py) alone:

  * every case has its constructed verdict, count and (exact family) transform, to the bit;
  * the named cause is the only gate that fires: `fired()` walks the gates of aligning_ref.worker WITHOUT stopping at the first one,
    and where the gate has a bound, the oracle accepts the same input with only that bound opened;
  * the extent and inlier witnesses are single: without the witness row the tight bound accepts, the count is 4;
  * the elimination, restated with the kernel's pivot rule, needs a row swap at each of columns 0, 1, 2 in some ordering.

Degeneracy band.  The kernel rejects a sample when a pivot of the 4 x 4 system [src 1] is <= 1e-13 x the largest |src| entry; the oracle
when |det [src 1]| < 1e-13 x that entry cubed.  Both reject exactly singular samples and accept well-conditioned ones; in between --
cond([src 1]) from about 1e6 up to numerical singularity -- the two criteria can disagree and cv2.estimateAffine3D, which neither
restates, is absent: parity is UNPINNED there.  `test_samples_keep_out_of_the_degeneracy_band` asserts that every sample any case uses
is exactly singular (integer determinant 0) or has cond < 1e6."""
import fractions
import itertools

import numpy as np
import pytest

import ransac_cases as rc
from oracle import aligning_ref


def _oracle(case):
    return aligning_ref.estimate9DTransform(case.src, case.dst, case.thres, case.ids, case.max_scale, case.min_scale, case.max_dims)[2]


def fired(case, h=0):
    """the gates of aligning_ref.worker that reject hypothesis h, all of them (the worker returns at the first)"""
    s4, d4 = case.src[case.ids[h]], case.dst[case.ids[h]]
    tf = aligning_ref.affine_from_4(s4, d4)
    if tf is None:
        return {'degenerate'}
    out = set()
    scales = np.linalg.norm(tf[:3, :3], axis=0)
    out |= {f'max_scale[{j}]' for j in range(3) if scales[j] > case.max_scale[j]}
    out |= {f'min_scale[{j}]' for j in range(3) if scales[j] < case.min_scale[j]}
    R = tf[:3, :3] / scales.reshape(1, 3)
    u, s, vh = np.linalg.svd(R)
    if s.min() < 0.8:
        out.add('sigma_min')
    if s.max() > 1.2:
        out.add('sigma_max')
    R = u @ vh
    if np.linalg.det(R) < 0:
        out.add('det')
    new_t = tf.copy(); new_t[:3, :3] = R @ np.diag(scales)
    if case.max_dims is not None:
        can = (np.linalg.inv(new_t) @ np.concatenate([case.dst, np.ones((case.N, 1))], 1).T).T[:, :3]
        ext = can.max(axis=0) - can.min(axis=0)
        out |= {f'max_dimensions[{i}]' for i in range(3) if ext[i] > case.max_dims[i]}
    return out


def _certify(case):
    outs = _oracle(case)
    for h, o in enumerate(outs):
        assert (o is not None) == bool(case.accept[h]), f'{case}[{h}]: oracle {"accepts" if o is not None else "rejects"}'
        f = fired(case, h)
        assert f == (set() if case.accept[h] else {case.cause}), f'{case}[{h}]: gates fired {f}, constructed cause {case.cause}'
        if o is None:
            continue
        if case.count is not None:
            assert o[0] == case.count[h], f'{case}[{h}]: oracle counts {o[0]}, constructed {case.count[h]}'
        if case.T is not None:
            assert np.array_equal(o[1], case.T), f'{case}[{h}]: the oracle transform is not the constructed one to the bit'
    r = case.relaxed()
    if r is not None:
        assert all(o is not None for o in _oracle(r)), f'{case}: opening only {list(case.relax)} does not flip the verdict'
    return outs


def test_scale_reflection_elimination_and_degenerate_cases():
    cases = rc.scale_cases() + rc.reflection_cases() + [rc.orderings()] + rc.degenerate_cases()
    assert len(rc.scale_cases()) == 12 and sum(c.accept.all() for c in rc.scale_cases()) == 6
    for c in cases:
        _certify(c)


def test_shear_cases_keep_their_margin():
    for case, (kind, c, ok, cause) in zip(rc.shear_cases(), rc.SHEARS):
        outs = _certify(case)
        tf = aligning_ref.affine_from_4(case.src[:4], case.dst[:4])
        s = np.linalg.svd(tf[:3, :3] / np.linalg.norm(tf[:3, :3], axis=0), compute_uv=False)
        lo, hi = rc.shear_sigmas(kind, c)
        assert abs(s.min() - lo) < 1e-12 and abs(s.max() - hi) < 1e-12
        assert min(abs(s.min() - 0.8), abs(s.max() - 1.2), abs(s.min() - 1.2), abs(s.max() - 0.8)) >= rc.SIGMA_MARGIN
        assert (s.min() < 0.8) == (cause == 'sigma_min') and (s.max() > 1.2) == (cause == 'sigma_max')
        if ok:           # no residual near the threshold: the count cannot depend on the last bits of T
            T = outs[0][1]
            errs = np.linalg.norm(case.src @ T[:3, :3].T + T[:3, 3] - case.dst, axis=-1)
            assert ((errs < case.thres / 2) | (errs > 2 * case.thres)).all() and 1 <= outs[0][0] <= 2


@pytest.mark.parametrize('N', rc.NS)
def test_extent_and_inlier_witnesses(N):
    assert rc.positions(600) == [4, 63, 64, 127, 128, 191, 192, 255, 256, 511, 599] and rc.positions(4) == []
    _certify(rc.all_inliers_case(N))
    for p in rc.positions(N):
        for above in (False, True):
            case = rc.inlier_case(N, p, above)
            outs = _certify(case)
            assert sorted(outs[0][2]) == [0, 1, 2, 3] + ([] if above else [p])
        for axis, end in itertools.product(range(3), ('max', 'min')):
            for case in rc.extent_cases(N, p, axis, end):
                _certify(case)
            for case in rc.extent_cases(N, p, axis, end, witness=False):       # without the witness row the tight bound accepts
                assert case.accept.all()
                _certify(case)


def _kernel_elimination_swaps(s4):
    """Gauss-Jordan of [src 1] with the kernel's pivot rule -> the columns at which M[c][c] == 0 forced a row swap"""
    M = np.concatenate([s4, np.ones((4, 1))], axis=1)
    swaps = []
    for c in range(4):
        piv = c + int(np.argmax(np.abs(M[c:, c])))
        if M[c, c] == 0.0:
            swaps.append(c)
        assert abs(M[piv, c]) > 0
        M[[c, piv]] = M[[piv, c]]
        M[c] /= M[c, c]
        for r in range(4):
            if r != c:
                M[r] -= M[r, c] * M[c]
    return swaps


def test_orderings_force_a_row_swap_at_every_column():
    case = rc.orderings()
    assert len(case.ids) == 24 and len({tuple(r) for r in case.ids}) == 24
    forced = set()
    for row in case.ids:
        forced |= set(_kernel_elimination_swaps(case.src[row]))
    assert {0, 1, 2} <= forced


def _exactly_singular(s4):
    M = [[fractions.Fraction(float(v)) for v in row] + [fractions.Fraction(1)] for row in s4]
    det = 0
    for perm in itertools.permutations(range(4)):
        sign = (-1) ** sum(perm[i] > perm[j] for i in range(4) for j in range(i + 1, 4))
        det += sign * M[0][perm[0]] * M[1][perm[1]] * M[2][perm[2]] * M[3][perm[3]]
    return det == 0


def test_samples_keep_out_of_the_degeneracy_band():
    rc.SAMPLES.clear()
    rc.scale_cases(); rc.shear_cases(); rc.reflection_cases(); rc.orderings(); rc.degenerate_cases()
    for N in rc.NS:
        rc.all_inliers_case(N)
        for p in rc.positions(N):
            rc.inlier_case(N, p, False); rc.extent_cases(N, p, 0, 'max')
    src, _, models = rc.selection_cloud()
    samples = rc.SAMPLES + [('selection', src[ids]) for ids, _, _ in models.values()]
    singular = 0
    for name, s4 in samples:
        if _exactly_singular(s4):
            singular += 1
            assert name.startswith('degenerate') or name == 'selection'
        else:
            assert np.linalg.cond(np.concatenate([s4, np.ones((4, 1))], axis=1)) < 1e6, name
    assert singular == 7


def test_mask_and_selection_inputs():
    for N in (1, 255, 256, 257):
        src, dst, T, mask = rc.mask_case(N)
        errs = np.linalg.norm(src @ T[:3, :3].T + T[:3, 3] - dst, axis=-1)
        assert np.array_equal((errs <= rc.THRES).astype(np.uint8), mask)
        assert set(np.unique(errs)) <= {0.0, rc.THRES, rc.JUST_ABOVE, rc.OUTLIER} and rc.THRES < rc.JUST_ABOVE < rc.THRES * (1 + 1e-11)
        assert (errs == rc.THRES).sum() == (N + 2) // 4 and (errs == rc.JUST_ABOVE).sum() == (N + 1) // 4
    src, dst, m = rc.selection_cloud()
    ids = np.array([m[k][0] for k in ('bad', 'c', 'a', 'b')])
    T, inl, outs = aligning_ref.estimate9DTransform(src, dst, rc.THRES, ids, rc.OPEN_MAX, rc.OPEN_MIN)
    assert [None if o is None else o[0] for o in outs] == [None, 5, 7, 7]
    assert np.array_equal(T, m['a'][1]) and not np.array_equal(m['a'][1], m['b'][1])        # equal counts: the first wins


# ---- the yardstick of ransac_cases.T_TOL -------------------------------------------------------------------------------------------
def _worker_T_longdouble(s4, d4):
    """the transform of aligning_ref.worker (affine through the sample, column scales, nearest rotation u @ vh, R diag(scales)) in
    np.longdouble: Gauss-Jordan with partial pivoting for the solve, Newton's iteration X <- (X + X^-T) / 2 for the orthogonal polar
    factor, which IS u @ vh."""
    L = np.longdouble
    M = np.concatenate([s4.astype(L), np.ones((4, 1), dtype=L), d4.astype(L)], axis=1)
    for c in range(4):
        piv = c + int(np.argmax(np.abs(M[c:, c])))
        M[[c, piv]] = M[[piv, c]]
        M[c] = M[c] / M[c, c]
        for r in range(4):
            if r != c:
                M[r] = M[r] - M[r, c] * M[c]
    X = M[:, 4:]
    A, t = X[:3].T.copy(), X[3].copy()
    sc = np.sqrt((A * A).sum(axis=0))
    R = A / sc

    def inv3(m):
        c = np.array([[m[(i + 1) % 3, (j + 1) % 3] * m[(i + 2) % 3, (j + 2) % 3] - m[(i + 1) % 3, (j + 2) % 3] * m[(i + 2) % 3, (j + 1) % 3]
                       for j in range(3)] for i in range(3)], dtype=L)          # cofactors
        return c.T / (m[0] * c[0]).sum()
    for _ in range(60):
        Rn = (R + inv3(R).T) / L(2)
        done = np.abs(Rn - R).max() < L(1e-19)
        R = Rn
        if done:
            break
    T = np.zeros((4, 4), dtype=L); T[3, 3] = 1
    T[:3, :3] = R * sc; T[:3, 3] = t
    return T


def random_problem():
    """the cloud, hypotheses and bounds of tests/test_aligning_gpu.py::test_hypotheses_and_best_transform_match_oracle"""
    import test_aligning_gpu as tg
    src, dst, _ = tg._problem(0)
    rng = np.random.default_rng(1)
    ids = np.stack([rng.choice(len(src), 4, replace=False) for _ in range(600)]).astype(np.int32)
    ids[5] = [7, 7, 8, 9]
    return src, dst, ids, [0.005, 0.005, 0.001], [0.05, 0.05, 0.05], np.array([1.2, 1.2, 1.2])


def test_tolerance_yardstick_oracle_against_longdouble():
    if np.finfo(np.longdouble).eps >= np.finfo(np.float64).eps:
        pytest.fail('np.longdouble is no wider than float64 here: the yardstick cannot be measured')
    src, dst, ids, min_s, max_s, max_d = random_problem()
    outs = aligning_ref.estimate9DTransform(src, dst, 0.003, ids, max_s, min_s, max_d)[2]
    gap = max(float(np.abs(o[1] - _worker_T_longdouble(src[ids[h]], dst[ids[h]])).max()) for h, o in enumerate(outs) if o is not None)
    print(f'MEASURED oracle vs longdouble, largest |dT| over {sum(o is not None for o in outs)} accepted hypotheses: {gap:.3e}')
    assert 0 < gap <= 4 * rc.ORACLE_LD_GAP and rc.T_TOL == 16 * max(rc.ORACLE_LD_GAP, rc.DEVICE_GAP)
