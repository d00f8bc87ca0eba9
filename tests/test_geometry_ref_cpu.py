"""The restatements of tests/geometry_ref.py are the oracles' operations, and its scenes reach the edges they are built for (CPU).

test_geometry_edges_gpu.py compares the kernels with geometry_ref bit for bit; this module is what makes that comparison mean
something: the restatements equal oracle/affordance_ref.py, grasp_sampler_ref.py and aligning_ref.py, points do lie exactly on
every boundary, every RANSAC gate has hypotheses on both sides, and the hypotheses a Jacobi / LAPACK difference could flip are few."""
import numpy as np
import pytest

import geometry_ref as G
from catgrasp_amd import synth
from oracle import affordance_ref, aligning_ref
from oracle import grasp_sampler_ref as gref

BOX_V = np.array([[G.LATTICE_EXTENT[0], 0, G.LATTICE_EXTENT[2]], [G.LATTICE_EXTENT[1], 0, G.LATTICE_EXTENT[3]]])     # a finger "mesh" with that extent


def _same_as_oracle(T44, pts, nrm, aff, V, sign, tol):
    c, m = G.finger_patch(T44[:3].reshape(12), pts, nrm, aff, (V[:, 0].min(), V[:, 0].max(), V[:, 2].min(), V[:, 2].max()), sign, tol)
    sp = affordance_ref.get_finger_contact_area(V, T44, pts, [0, sign, 0], nrm, tol)
    assert (sp is None) == (m is None)
    assert c == (0 if sp is None else len(sp))
    return m is not None


def test_finger_patch_is_the_oracle_on_the_lattice_scene_which_reaches_every_edge():
    s = G.lattice_scene()
    pts, nrm, aff = s['pts'], s['nrm'], s['aff']
    assert len(pts) == 130 and len(s['T']) == 480
    xmin, xmax, zmin, zmax = G.LATTICE_EXTENT
    on_face = at_tol = dot0 = valid = split = 0
    with np.errstate(invalid='ignore'):                                  # the oracle normalises a zero normal to NaN; NaN > 0 is False
        for T12 in s['T']:
            ok = []
            for sign in (1, -1):
                ok.append(_same_as_oracle(G.to44(T12), pts, nrm, aff, BOX_V, sign, G.LATTICE_TOL))
                r = G.finger_patch_detail(T12, pts, nrm, aff, G.LATTICE_EXTENT, sign, G.LATTICE_TOL)
                w = r['within']
                on_face += bool((w & ((r['qx'] == xmin) | (r['qx'] == xmax) | (r['qz'] == zmin) | (r['qz'] == zmax))).any())
                if r['patch'] is not None:
                    at_tol += bool((r['patch'] & (r['d'] == G.LATTICE_TOL)).any())
                    dot0 += r['dot'] == 0.0
                valid += ok[-1]
            split += ok[0] != ok[1]
    print(f'lattice scene: on a face {on_face}, at tol {at_tol}, dot 0 {dot0}, valid {valid} of 960; one finger of two valid {split} of 480')
    assert min(on_face, at_tol, dot0, valid, 960 - valid, split) >= 50


def test_inverse_of_lattice_poses_is_exact():
    """The wrapper hands the kernel inv(grasp pose); for a signed permutation with a dyadic translation LAPACK's inverse is exact, so a
    caller with such poses runs the kernel on exactly the rows the GPU cases state."""
    exact = 0
    for T12 in G.lattice_scene()['T']:
        T = G.to44(T12)
        pose = np.eye(4); pose[:3, :3] = T[:3, :3].T; pose[:3, 3] = -(T[:3, :3].T @ T[:3, 3])
        exact += np.array_equal(np.linalg.inv(pose), T)
    assert exact == 480


def test_tie_scenes_tie():
    for gap in (64, 1):
        for swapped in (False, True):
            pts, nrm, aff, T12 = G.tie_scene(gap, swapped)
            r = G.finger_patch_detail(T12, pts, nrm, aff, G.LATTICE_EXTENT, 1, G.LATTICE_TOL)
            assert r['first'] == 3 and r['d'][3] == 0.0 and r['d'][3 + gap] == 0.0 and (r['d'] == 0.0).sum() == 2
            assert (r['count'] > 0) == swapped
            assert _same_as_oracle(G.to44(T12), pts, nrm, aff, BOX_V, 1, G.LATTICE_TOL) == swapped


def test_finger_patch_is_the_oracle_on_the_random_scene():
    pts, nrm, aff, finger_V, fig, poses = G.random_affordance_scene(1500, 200)
    valid = 0
    for pose in poses:
        cif = np.linalg.inv(fig) @ np.linalg.inv(pose)
        for V, sign in zip(finger_V, (-1, 1)):
            valid += _same_as_oracle(cif, pts, nrm, aff, V, sign, 0.005)
    assert valid >= 50 and 2 * len(poses) - valid >= 5


def test_center_y_is_the_oracle():
    s = G.lattice_scene()
    poses = np.array([G.to44(T) for T in s['T'][::7]])
    got = G.center_y(poses, s['pts'])
    assert np.array_equal(got, gref.center_between_gripper(poses, s['pts']))
    assert (got != poses).any(axis=(1, 2)).sum() > len(poses) // 2                     # the shift is not 0
    rng = np.random.default_rng(5)
    ob = synth.make_scene(1, 300, 7)[0]
    poses = synth.make_candidates(ob, 40, rng)
    assert np.abs(G.center_y(poses, ob['xyz']) - gref.center_between_gripper(poses, ob['xyz'])).max() < 1e-12


def test_nearest_first_is_the_first_minimum():
    ref = np.array([[0, 0, 0], [1, 0, 0], [0, 0, 0], [1, 0, 0.0]])
    assert G.nearest_first([[0.1, 0, 0], [0.9, 0, 0], [0.5, 0, 0]], ref).tolist() == [0, 1, 0]


def test_ransac_problem_is_the_one_of_the_aligning_test():
    import test_aligning_gpu
    for a, b in zip(G.ransac_problem(7, 65, 0.15, 1e-4), test_aligning_gpu._problem(7, 65, 0.15, 1e-4)):
        assert np.array_equal(a, b)


@pytest.mark.parametrize('n', G.RANSAC_N)
def test_ransac_gate_census(n):
    """Every gate of the hypothesis test rejects and passes at least 5 of the 400 hypotheses, and the hypotheses that sit within 1e-9
    of a threshold -- the only ones on which the kernel's Jacobi and the oracle's LAPACK may disagree, and which the GPU comparison
    may therefore leave out -- are at most 1 % (in fact none)."""
    line = []
    for dims in G.RANSAC_DIMS:
        c = G.ransac_case(n, dims)
        st = c['stage']
        assert np.array_equal(st == '', c['ref_counts'] >= 0)              # the gate walk is the oracle's worker
        census = {k: int((st == k).sum()) for k in ('degenerate', 'scale', 'sv', 'det', 'extent', '')}
        line.append(f'max_dimensions {dims}: {census}, near a threshold {int(c["near"].sum())}')
        assert census['scale'] >= 5 and G.RANSAC_H - census['scale'] >= 5
        assert census['sv'] >= 5 and census[''] >= 5
        if dims == 1.02:
            assert census['extent'] >= 5
        assert c['near'].mean() <= 0.01
    print(f'N = {n}: ' + '; '.join(line))


def test_exact_tetrahedron_in_the_oracle():
    src, dst = G.tetra_problem()
    two = np.array([2.0, 2, 2])
    T = np.eye(4); T[:3, :3] *= 2; T[:3, 3] = G.TETRA_T
    ids = np.array([[0, 1, 2, 3]])
    assert np.array_equal(G.similarity_residuals(src, dst, T), [0, 0, 0, 0, 0.25, 0.25 + 2.0 ** -40, 0.25])
    for thres, cnt in ((0.25, 6), (0.25 - 2.0 ** -40, 4)):
        T_ref, inl, outs = aligning_ref.estimate9DTransform(src, dst, thres, ids, two, two)
        assert np.array_equal(T_ref, T) and outs[0][0] == cnt and int(G.similarity_inliers(src, dst, T, thres).sum()) == cnt
    assert aligning_ref.estimate9DTransform(src, dst, 0.25, ids, two - 2.0 ** -40, two)[0] is None
    src, dst, ids = G.degenerate_problem()
    assert aligning_ref.estimate9DTransform(src, dst, 0.25, ids, [99.0] * 3, [0.0] * 3)[0] is None
    assert aligning_ref.estimate9DTransform(src, dst, 0.25, np.array([[0, 1, 2, 6]]), [99.0] * 3, [0.0] * 3)[0] is not None


def test_four_point_problem_and_mirrored_problem_in_the_oracle():
    src, dst, ids = G.four_point_problem()
    for dims in G.RANSAC_DIMS:
        st, near = G.ransac_gates(src, dst, ids, G.RANSAC_THRES, G.MIN_SCALE, G.MAX_SCALE, None if dims is None else np.array([dims] * 3))
        assert st[0] == '' and not near[0]
    c = G.ransac_case(63, None)
    src = c['src'] * np.array([-1.0, 1, 1])
    st, near = G.ransac_gates(src, c['dst'], c['ids'][:200], G.RANSAC_THRES, G.MIN_SCALE, G.MAX_SCALE, None)
    print('mirrored:', {k: int((st == k).sum()) for k in set(st)})
    assert (st != '').all() and (st == 'det').sum() >= 5 and not near.any()


def test_cone_cloud_reaches_its_edges():
    """In the oracle: the neighbour at exactly r is used (no doubling at point 0), cluster B doubles the radius exactly once, and
    enough blocks have a unique minor direction to be compared whole."""
    for P, K, radii in ((2, 1, [1]), (63, 4, [1, 2, 2, 2]), (64, 5, [1, 2, 2, 2, 2]), (65, 5, [1, 2, 2, 2, 2])):
        pts, nrm, ids = G.cone_cloud(P)
        s = gref.ConeSampler(r_ball=G.CONE_R, inplane_step_deg=G.CONE_STEP_DEG, **G.CONE_KW)
        unique = 0
        for k, sid in enumerate(ids[:K]):
            out = s.sample_one_surface_point(pts[sid], nrm[sid], pts, nrm, G.CONE_SPHERE)
            assert out.shape == ((1 + 4 * 4) * 3, 4, 4) and np.isfinite(out).all()
            assert s.r_ball == radii[k] * G.CONE_R
            ev = s.last_eigvals
            unique += ev[1] - ev[0] > 1e-3 * max(ev[2], 1e-12)
        assert unique >= (0 if P == 2 else 3)
