"""CPU proof of tests/prep_ref.py, the host reference of tests/test_prep_kernels_gpu.py and of the batched SDF check:
  * every float32 chain lies within its derived bound of its float64 reference (the worst ratio is printed: the bounds are not
    vacuous), and the seeded cases reach the branches their names promise (read off a host restatement of the staged kernel's
    slice logic);
  * defects planted in the host restatements fail the same comparison functions the GPU tests apply."""
import numpy as np
import pytest

import dense_ref as R
import prep_ref as Q
from oracle import sdf_ref

f32 = np.float32

GRASP_CASES = ['S1', 'S2', 'S3', 'S4-64', 'S4-64-nomean', 'S4-128', 'S4-128-nomean', 'S4-1088', 'S4-1088-nomean', 'P1', 'P1-nomean',
               'P2', 'P3', 'P4', 'X']


def _chain(case, **kw):
    return Q.grasp_chain_points(case['T12'], case['xyz32'][case['ids']], case['nrm32'][case['ids']], case['mean32'], case['inv_std32'], **kw)


# ------------------------------------------------------------------------------------------------------ build_grasp_input
@pytest.mark.parametrize('name', GRASP_CASES)
def test_grasp_chain_within_bound_of_float64(name):
    case = Q.grasp_case(name)
    assert case['ids'].min() >= 0 and case['ids'].max() < len(case['xyz32'])
    ratio = Q.check_grasp(case, _chain(case), name)
    print(f'{name}: worst error / bound {ratio:.3f}')
    assert 0.05 < ratio <= 1.0


def test_staged_restatement_is_the_plain_gather_and_cases_reach_their_branches():
    paths = {}
    for name in ('S1', 'S2', 'S3'):
        case = Q.grasp_case(name)
        p, n, trace = Q.staged_gather(case['xyz32'], case['nrm32'], case['ids'], len(case['xyz32']))
        assert np.array_equal(p, case['xyz32'][case['ids']]) and np.array_equal(n, case['nrm32'][case['ids']])
        paths[name] = (case, trace, ''.join(t['path'][0] for t in trace))
    case, trace, s = paths['S1']
    assert len(case['ids']) % Q.BGI_CPB != 0 and len(case['xyz32']) < Q.BGI_CAP and s.count('r') >= 10 and 'g' not in s
    case, trace, s = paths['S2']
    assert len(set(case['sizes'])) == 3 and any(n * 3 % 4 for n in case['sizes'])
    assert {int(b) % 4 for b in case['base']} >= {0, 1, 3}
    staged = [t for t in trace if t['path'] == 'stage']
    assert any(t['lo'] % 4 for t in staged) and any(t['tail'] for t in staged)
    # a workgroup's candidates cross an object boundary, so the slice is staged again inside the workgroup
    og = case['obj_of_g']
    assert any(og[g] != og[g - 1] and trace[g]['path'] == 'stage' for g in range(len(og)) if g % Q.BGI_CPB)
    case, trace, s = paths['S3']
    assert s[:8] == 'srgrsgrs' and s[8:] == 'gsgsgs', s           # staged, global, the old slice again, ... inside one workgroup
    assert trace[11]['hi'] - (trace[11]['lo'] & ~3) + 1 == Q.BGI_CAP and trace[11]['path'] == 'stage'
    assert trace[12]['hi'] - (trace[12]['lo'] & ~3) + 1 == Q.BGI_CAP + 1 and trace[12]['path'] == 'global'
    # the plain-kernel cases are the ones the launcher sends there
    for name, odd_total in (('P1', False), ('P2', False), ('P3', True)):
        G, n_pts = Q.grasp_case(name)['ids'].shape
        assert n_pts % 64 != 0 and (G * n_pts) % 2 == odd_total
    assert Q.grasp_case('P1')['ids'].shape[1] % 2 == 0 and Q.grasp_case('P2')['ids'].shape[1] % 2 == 1


@pytest.mark.parametrize('defect', ['off_by_one', 'no_granule'])
def test_planted_slice_defects_fail(defect):
    case = Q.grasp_case('S2')
    p, n, _ = Q.staged_gather(case['xyz32'], case['nrm32'], case['ids'], len(case['xyz32']), defect=defect)
    bad = Q.grasp_chain_points(case['T12'], p, n, case['mean32'], case['inv_std32'])
    with pytest.raises(AssertionError):
        Q.check_grasp(case, bad, defect)
    if defect == 'no_granule':      # only the objects whose base is off the 4-point granule notice
        good = _chain(case)
        wrong = {case['obj_of_g'][g] for g in range(len(bad)) if not np.array_equal(bad[g], good[g])}
        assert wrong == {k for k, b in enumerate(case['base']) if b % 4}


@pytest.mark.parametrize('kw', [{'normal_plus_t': True}, {'fused_norm': True}])
def test_planted_chain_defects_fail(kw):
    case = Q.grasp_case('S4-128')
    with pytest.raises(AssertionError):
        Q.check_grasp(case, _chain(case, **kw), str(kw))
    if 'fused_norm' in kw:          # a fused normaliser stays inside the float64 bound: only the bitwise comparison sees it
        ref = Q.grasp_ref64(case)
        assert R.check_bound(_chain(case, **kw), ref, Q.grasp_bound(case, ref), 'fused') <= 1.0


# ----------------------------------------------------------------------------------------------------- build_nunocs_input
@pytest.mark.parametrize('with_mean', [False, True])
@pytest.mark.parametrize('n_pts', [1, 63, 1024, 1025, 8192])
def test_nunocs_chain_within_bound_of_float64(n_pts, with_mean):
    case = Q.nunocs_case(5, n_pts, with_mean)
    out = Q.nunocs_input_chain(case['xyz32'], case['nrm32'], case['ids'], case['mean32'], case['inv_std32'])
    ratio = Q.check_nunocs(case, out, f'nunocs {n_pts}')
    print(f'nunocs n_pts {n_pts} mean {with_mean}: worst error / bound {ratio:.3f}')
    assert 0.05 < ratio <= 1.0
    if n_pts > 1:                   # the largest extent is on every axis in turn
        assert {int(np.argmax(np.ptp(case['xyz32'][i], axis=0))) for i in case['ids']} == {0, 1, 2}


def test_nunocs_divisor_without_epsilon_fails_on_a_degenerate_cloud():
    case = Q.nunocs_case(5, 1024, True, degenerate=True)
    out = Q.nunocs_input_chain(case['xyz32'], case['nrm32'], case['ids'], case['mean32'], case['inv_std32'])
    assert np.isfinite(out).all()                               # 0 / 1e-15f = 0
    assert not np.isfinite(Q.nunocs_bound(case, Q.nunocs_ref64(case))[0, :, :3]).any()       # no float64 bound: bytes alone
    Q.check_nunocs(case, out, 'degenerate')
    bad = Q.nunocs_input_chain(case['xyz32'], case['nrm32'], case['ids'], case['mean32'], case['inv_std32'], no_eps=True)
    with pytest.raises(AssertionError):
        Q.check_nunocs(case, bad, 'no epsilon')


# ------------------------------------------------------------------------------------------------------------- softmax_pg
def _softmax_f32(x, last_max=False):
    """softmax_pg_kernel on the host in float32 (numpy's expf in place of the device's)."""
    x = np.asarray(x, f32)
    B, C = x.shape
    e = np.exp((x - x.max(axis=1, keepdims=True)).astype(f32)).astype(f32)
    s = np.zeros(B, f32)
    for k in range(C):
        s = (s + e[:, k]).astype(f32)
    p = (e * (f32(1) / s)[:, None]).astype(f32)
    pg = np.zeros(B, f32)
    for k in range(C):
        pg = R.fmaf(p[:, k], f32(k), pg)
    label = (C - 1 - p[:, ::-1].argmax(axis=1)) if last_max else p.argmax(axis=1)
    return p, label.astype(np.int32), p[np.arange(B), label], (pg / f32(C)).astype(f32)


@pytest.mark.parametrize('C', [1, 2, 10, 33])
def test_softmax_check_passes_a_faithful_kernel_and_fails_the_last_maximum(C):
    x, planted = Q.softmax_case(257, C)
    worst = Q.check_softmax(x, planted, *_softmax_f32(x), 1e-6, f'softmax C {C}')
    print(f'softmax C {C}: worst |p - float64| {worst:.2f} u')
    if C >= 2:
        assert 1 in planted and 2 in planted and planted[3] == C - 1
        with pytest.raises(AssertionError):
            Q.check_softmax(x, planted, *_softmax_f32(x, last_max=True), 1e-6, 'last maximum')


def test_softmax_check_fails_without_the_max_subtraction():
    x, planted = Q.softmax_case(8, 10)
    with np.errstate(over='ignore', invalid='ignore'):
        e = np.exp(x).astype(f32)
        p = (e / e.sum(axis=1, keepdims=True)).astype(f32)
    lab = np.nan_to_num(p).argmax(axis=1)
    with pytest.raises(AssertionError):
        Q.check_softmax(x, planted, p, lab, p[np.arange(8), lab], np.zeros(8, f32), 1e-6, 'no max subtraction')


# --------------------------------------------------------------------------------------------------------------------- sdf
def test_sdf_planted_candidates_and_defects():
    grid, xf, pts, exp, names = Q.sdf_planted_case()
    assert len(xf) % 4 != 0 and len(pts) % 64 != 0
    got = Q.sdf_inside_chain(grid, xf, pts)
    assert np.array_equal(got, exp), [n for n, a, b in zip(names, got, exp) if a != b]
    gx = Q.sdf_grid_coords(xf, pts)[0]
    assert np.signbit(np.rint(gx[names.index('rounds-to-minus-zero')])).any() and (np.rint(gx) == 0).any()       # a real -0
    for defect, must in (('half_up', {'half-even-down', 'half-even-down-outside'}), ('clamp_first', {'rounds-to-nx', 'beyond-x-low', 'beyond-z-high'})):
        bad = Q.sdf_inside_chain(grid, xf, pts, **{defect: True})
        assert must <= {n for n, a, b in zip(names, bad, exp) if a != b}
    # the float32 coordinates lie within the coordinate bound of float64 on general candidates
    grid, xf, pts = Q.sdf_random_case(200, 333)
    A = xf.astype(np.float64).reshape(-1, 3, 4)
    p = pts.astype(np.float64)
    g64 = np.einsum('eij,pj->epi', A[:, :, :3], p) + A[:, None, :, 3]
    bound = Q.gamma(4) * (np.einsum('eij,pj->epi', np.abs(A[:, :, :3]), np.abs(p)) + np.abs(A[:, None, :, 3]))
    ratio = R.check_bound(np.stack(Q.sdf_grid_coords(xf, pts), axis=-1), g64, bound, 'sdf coordinates')
    print(f'sdf coordinates: worst error / bound {ratio:.3f}')
    assert 0.05 < ratio <= 1.0


@pytest.mark.parametrize('E,sigma,seed', [(64, 0.03, 1), (2000, 0.03, 2), (2000, 0.02, 3)])
def test_sdf_float64_decides_the_batched_check(E, sigma, seed):
    """The inputs of test_sdf_gpu.py::test_batched_candidate_inside_check (the first and the last case are the ones it runs, the
    last cut to its first 500 candidates): float64 forces nearly every candidate, so the GPU test needs no allowance."""
    data, origin, res = sdf_ref.box_sdf_grid([-0.01, -0.004, -0.007], [0.012, 0.006, 0.003], 0.001, 5)
    Twg = np.eye(4)
    Twg[:3, :3] /= res
    Twg[:3, 3] = -origin / res
    poses, pts = Q.sdf_pose_case(E, sigma, seed)
    cls, oracle = Q.sdf_classify(data, Twg, poses, pts)
    print(f'E {E} sigma {sigma}: {int((cls < 0).sum())} undecided, inside share {oracle.mean():.3f}')
    assert (cls < 0).mean() <= 0.01 and 0.2 < oracle.mean() < 0.8
    assert np.array_equal(oracle[cls >= 0], cls[cls >= 0] == 1)            # what is forced is what the oracle says
    Q.check_sdf_batch(oracle, cls, 'oracle')
    flipped = oracle.copy()
    flipped[np.nonzero(cls >= 0)[0][0]] ^= True                              # one unexplained flip is a failure
    with pytest.raises(AssertionError):
        Q.check_sdf_batch(flipped, cls, 'one flip')
