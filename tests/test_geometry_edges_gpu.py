"""The float64 grasp-geometry kernels (csrc/affordance.hip, conesampler.hip, ransac.hip) at their edges.

Inputs on a dyadic lattice with signed-permutation rotations make every product and sum of these kernels exact (the library is built
without FMA contraction), so the kernel and the plain numpy restatement of tests/geometry_ref.py agree in every bit, and a point can
sit exactly ON each boundary: `<` for `<=`, a wrong tie rule, an idle lane or wave that leaks into a reduction, or a grid-stride loop
that runs once changes an integer count.  No tolerance is involved in those cases.  test_geometry_ref_cpu.py pins the restatements to
the oracles and asserts that the scenes do reach the edges.  Where the kernel and the oracle differ by construction (Jacobi against
LAPACK, general rigid poses) the bars of the existing tests hold: 1e-12 / 1e-8 for the cone sampler, 1e-9 for centring and RANSAC."""
import ctypes

import numpy as np
import pytest

import geometry_ref as G
from oracle import aligning_ref
from oracle import grasp_sampler_ref as gref

pytestmark = pytest.mark.gpu


def _d(a, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _bits_equal(got, exp):
    """Same NaN pattern, and every other value the same 64 bits."""
    got, exp = np.ascontiguousarray(got, dtype=np.float64), np.ascontiguousarray(exp, dtype=np.float64)
    nan = np.isnan(exp)
    return got.shape == exp.shape and np.array_equal(np.isnan(got), nan) and np.array_equal(got[~nan].view(np.uint64), exp[~nan].view(np.uint64))


# ------------------------------------------------------------------------------------------------------------------------------
# cg_grasp_affordance

def _affordance(dev, T12, pts, nrm, aff, extents, signs, tol):
    """cg_grasp_affordance on exactly these cam_in_finger rows.  -> (p_t_given_g (G,), counts (G, n_fingers))."""
    import torch
    from catgrasp_amd import _lib as L
    T12 = np.asarray(T12, dtype=np.float64).reshape(-1, 12)
    n, nf = len(T12), len(signs)
    out = torch.full((n,), -7.0, dtype=torch.float64, device=dev)
    counts = torch.full((n, nf), -7, dtype=torch.int32, device=dev)
    E = (ctypes.c_double * (4 * nf))(*[float(v) for e in extents for v in e])
    S = (ctypes.c_int * nf)(*signs)
    d_T, d_pts, d_nrm, d_aff = _d(T12, dev), _d(pts, dev), _d(nrm, dev), _d(aff, dev)       # named: alive until the kernel has run
    L.check(L.lib().cg_grasp_affordance(L._p(d_T), n, L._p(d_pts), L._p(d_nrm), L._p(d_aff), len(pts), nf, E, S, float(tol), L._p(out), L._p(counts),
                                        L._stream()), 'cg_grasp_affordance')
    return out.cpu().numpy(), counts.cpu().numpy()


def _expected_affordance(T12, pts, nrm, aff, extents, signs, tol):
    r = [G.p_t_given_g(T, pts, nrm, aff, extents, signs, tol) for T in np.asarray(T12).reshape(-1, 12)]
    return np.array([v for v, _ in r]), np.array([c for _, c in r], dtype=np.int32).reshape(len(r), len(signs))


@pytest.mark.parametrize('P', [1, 63, 64, 65, 130])
def test_affordance_bit_exact_on_the_lattice(cuda_device, P):
    """480 poses x {both fingers, +y finger alone, -y finger alone} on the first P lattice points: points on the faces of the finger
    box, at exactly surface_tol, first-touched normals exactly perpendicular to grip_dir, P below and at the wave width."""
    s = G.lattice_scene()
    pts, nrm, aff = s['pts'][:P], s['nrm'][:P], s['aff'][:P]
    for signs in ((1, -1), (1,), (-1,)):
        ext = [G.LATTICE_EXTENT] * len(signs)
        got, cnt = _affordance(cuda_device, s['T'], pts, nrm, aff, ext, signs, G.LATTICE_TOL)
        exp, exp_cnt = _expected_affordance(s['T'], pts, nrm, aff, ext, signs, G.LATTICE_TOL)
        assert np.array_equal(cnt, exp_cnt), f'{(cnt != exp_cnt).any(axis=1).sum()} of 480 poses differ in a contact count'
        assert _bits_equal(got, exp)
        if P == 130 and len(signs) == 2:                  # one finger rejected, the other valid: the mean is the valid finger's alone
            assert ((exp_cnt[:, 0] > 0) != (exp_cnt[:, 1] > 0)).sum() >= 50


def test_affordance_empty_box_is_nan(cuda_device):
    s = G.lattice_scene()
    T = s['T'][:24].copy(); T[:, 3] += 10.0               # no point inside the x extent
    got, cnt = _affordance(cuda_device, T, s['pts'], s['nrm'], s['aff'], [G.LATTICE_EXTENT] * 2, (1, -1), G.LATTICE_TOL)
    assert np.isnan(got).all() and (cnt == 0).all()


@pytest.mark.parametrize('gap', [64, 1])
@pytest.mark.parametrize('swapped', [False, True])
def test_affordance_first_toucher_tie(cuda_device, gap, swapped):
    """Two coincident first touchers with opposite normals: the one with the smaller index decides (the reference's argmin).
    gap 64: same lane, the lane-local scan decides; gap 1: two lanes, the butterfly's index rule decides."""
    pts, nrm, aff, T12 = G.tie_scene(gap, swapped)
    got, cnt = _affordance(cuda_device, T12, pts, nrm, aff, [G.LATTICE_EXTENT], (1,), G.LATTICE_TOL)
    exp, exp_cnt = _expected_affordance(T12, pts, nrm, aff, [G.LATTICE_EXTENT], (1,), G.LATTICE_TOL)
    assert (exp_cnt[0, 0] > 0) == swapped and np.isnan(exp[0]) == (not swapped)
    assert np.array_equal(cnt, exp_cnt) and _bits_equal(got, exp)


def test_affordance_grid_stride(cuda_device):
    """G = 16384 + 5: the grid is capped at 4096 blocks of 4 poses, so the loop body runs a second time, in a block with one live wave."""
    s = G.lattice_scene()
    n = 16384 + 5
    pts, nrm, aff = s['pts'][:70], s['nrm'][:70], s['aff'][:70]
    ext = [G.LATTICE_EXTENT] * 2
    exp, exp_cnt = _expected_affordance(s['T'], pts, nrm, aff, ext, (1, -1), G.LATTICE_TOL)
    row = np.arange(n) % 480                                # 16384 % 480 != 0: a row that got the result of row - 16384 is wrong
    got, cnt = _affordance(cuda_device, s['T'][row], pts, nrm, aff, ext, (1, -1), G.LATTICE_TOL)
    assert np.array_equal(cnt, exp_cnt[row]) and _bits_equal(got, exp[row])


def test_affordance_general_poses_small_cloud(cuda_device):
    """The bar of test_affordance_gpu.py (counts equal, values within 1e-12 of the oracle) on general rigid poses at P = 65."""
    from scipy.spatial import cKDTree
    from catgrasp_amd import affordance
    from oracle import affordance_ref
    pts, nrm, aff, finger_V, fig, poses = G.random_affordance_scene(65, 400)
    grip_dirs = [[0, -1, 0], [0, 1, 0]]
    model = affordance.AffordanceModel(pts, nrm, pts, aff, device=cuda_device)
    got, counts = affordance.compute_grasp_affordance(model, poses, fig, finger_V, grip_dirs, 0.005, return_counts=True)
    kd = cKDTree(pts)
    ref = [affordance_ref.grasp_affordance(p, fig, pts, nrm, aff, kd, grip_dirs, finger_V, 0.005) for p in poses]
    ref_v = np.array([r[0] for r in ref]); ref_c = np.array([r[1] for r in ref])
    ok = ~np.isnan(ref_v)
    assert ok.sum() > 50 and (ref_c == 0).sum() > 5
    assert np.array_equal(np.isnan(got), ~ok) and np.array_equal(counts, ref_c)
    assert np.abs(got[ok] - ref_v[ok]).max() < 1e-12


# ------------------------------------------------------------------------------------------------------------------------------
# cg_nearest_neighbor

def _nearest(dev, query, ref):
    import torch
    from catgrasp_amd import _lib as L
    idx = torch.full((len(query),), -7, dtype=torch.int32, device=dev)
    d_query, d_ref = _d(query, dev), _d(ref, dev)
    L.check(L.lib().cg_nearest_neighbor(L._p(d_query), len(query), L._p(d_ref), len(ref), L._p(idx), L._stream()), 'cg_nearest_neighbor')
    return idx.cpu().numpy()


@pytest.mark.parametrize('R', [1, 63, 64, 65, 200])
def test_nearest_neighbor_equals_first_minimum(cuda_device, R):
    """Random float64 data: the kernel's distance is the same operations in the same order as nearest_first, so every index agrees."""
    rng = np.random.default_rng(R)
    ref = rng.normal(size=(R, 3))
    for Q in (1, 5, 16384 + 5):
        query = rng.normal(size=(Q, 3))
        assert np.array_equal(_nearest(cuda_device, query, ref), G.nearest_first(query, ref))


def test_nearest_neighbor_ties(cuda_device):
    """Lattice reference points, many of them repeated (among them 3 = 67: one lane, and 3 = 4: neighbouring lanes), and queries on
    the half lattice, each at exactly the same distance from several reference points: the smallest index wins."""
    rng = np.random.default_rng(9)
    ref = rng.integers(-2, 3, (130, 3)) / 4.0
    ref[3] = ref[4] = ref[67] = (0.25, -0.5, 0.75)
    ref[100] = ref[36] = (-0.75, 0.75, 0.25)                # lane 36, second then first round
    query = np.concatenate([ref[[3, 100]], rng.integers(-5, 6, (400, 3)) / 8.0])
    exp = G.nearest_first(query, ref)
    assert exp[0] == 3 and exp[1] == 36
    d2 = ((ref[None] - query[:, None]) ** 2).sum(axis=2)
    assert ((d2 == d2.min(axis=1, keepdims=True)).sum(axis=1) > 1).sum() > 300          # most queries are tied
    assert np.array_equal(_nearest(cuda_device, query, ref), exp)


# ------------------------------------------------------------------------------------------------------------------------------
# cone sampler

def _cone_blocks_match(got, pts, nrm, ids, sph, radii_units):
    """Every block of `got` against the oracle walking the same sample points: eigenvector-independent part to 1e-12, whole block to
    1e-8 for one of the two eigenvector signs where the minor direction is unique.  -> number of blocks compared whole."""
    n_depth = len(np.arange(0, G.CONE_KW['hand_depth'], G.CONE_KW['approach_step']))
    per = (1 + len(sph) * 4) * n_depth
    assert got.shape == (len(ids) * per, 4, 4) and got.dtype == np.float64
    s0 = gref.ConeSampler(r_ball=G.CONE_R, inplane_step_deg=G.CONE_STEP_DEG, **G.CONE_KW)
    s1 = gref.ConeSampler(r_ball=G.CONE_R, inplane_step_deg=G.CONE_STEP_DEG, **G.CONE_KW)
    whole = 0
    for k, sid in enumerate(ids):
        blk = got[k * per:(k + 1) * per]
        r0 = s0.sample_one_surface_point(pts[sid], nrm[sid], pts, nrm, sph, flip_minor=False)
        r1 = s1.sample_one_surface_point(pts[sid], nrm[sid], pts, nrm, sph, flip_minor=True)
        assert s0.r_ball == radii_units[k] * G.CONE_R
        assert np.abs(blk[:n_depth, :3, 0] - r0[:n_depth, :3, 0]).max() < 1e-12 and np.abs(blk[:n_depth, :3, 3] - r0[:n_depth, :3, 3]).max() < 1e-12
        ev = s0.last_eigvals
        if ev[1] - ev[0] > 1e-3 * max(ev[2], 1e-12):
            e = min(np.abs(blk - r0).max(), np.abs(blk - r1).max())
            assert e < 1e-8, (k, e)
            whole += 1
    return whole


@pytest.mark.parametrize('P,K', [(2, 1), (63, 4), (64, 5), (65, 5), (65, 1)])
@pytest.mark.parametrize('S', [4, 0])
def test_cone_sampler_on_the_built_cloud(cuda_device, P, K, S):
    """Neighbours at exactly r and exactly 2r, a duplicate of the sample point, a zero normal, the normal (1,-1,0) whose outer product
    sums to 0; approach directions +x, -x (the identity branch), +z and one 2^-20 off -x; 4 in-plane rotations of 50 degrees."""
    from catgrasp_amd import grasp_sampler
    pts, nrm, ids = G.cone_cloud(P)
    ids = ids[:K]
    sph = G.CONE_SPHERE[:S]
    info = {}
    got = grasp_sampler.cone_grasp_poses(pts, nrm, ids, sph, G.CONE_R, inplane_step_deg=G.CONE_STEP_DEG, info=info, device=cuda_device, **G.CONE_KW)
    units = [1, 2, 2, 2, 2][:K]
    # the neighbour at exactly r counts (no doubling at the first point); cluster B doubles the radius once, and for good
    assert np.array_equal(info['radii'], np.array(units) * G.CONE_R)
    whole = _cone_blocks_match(got, pts, nrm, ids, sph, units)
    assert whole >= (3 if K >= 4 else 0)


def _center(dev, poses, pts):
    from catgrasp_amd import _lib as L
    d_poses = _d(np.asarray(poses, dtype=np.float64).reshape(-1, 16), dev)
    d_pts = _d(pts, dev)
    L.check(L.lib().cg_center_grasps(L._p(d_poses), d_poses.shape[0], L._p(d_pts), len(pts), L._stream()), 'cg_center_grasps')
    return d_poses.cpu().numpy().reshape(-1, 4, 4)


@pytest.mark.parametrize('P', [1, 63, 64, 65])
def test_centring_bit_exact_on_the_lattice(cuda_device, P):
    """cg_center_grasps on signed-permutation poses with dyadic translations (the sampler's wrapper centres only poses it made itself,
    so the entry point is called directly): G = 16384 + 5 runs the grid-stride loop twice."""
    s = G.lattice_scene()
    pts = s['pts'][:P]
    base = np.array([G.to44(T) for T in s['T']])
    exp = G.center_y(base, pts)
    n = 16384 + 5 if P == 65 else 480
    row = np.arange(n) % 480
    if n > 480:
        assert (exp[row][16384:] != base[row][16384:]).any(axis=(1, 2)).all()           # the last rows do move
    got = _center(cuda_device, base[row], pts)
    assert np.array_equal(got.view(np.uint64), exp[row].view(np.uint64))


def test_centring_general_poses(cuda_device):
    from catgrasp_amd import synth
    ob = synth.make_scene(1, 65, 7)[0]
    poses = synth.make_candidates(ob, 50, np.random.default_rng(5))
    assert np.abs(_center(cuda_device, poses, ob['xyz']) - gref.center_between_gripper(poses, ob['xyz'])).max() < 1e-9


# ------------------------------------------------------------------------------------------------------------------------------
# RANSAC

def _ransac(dev, src, dst, ids, thres, min_s, max_s, max_d):
    """cg_ransac_9d; max_d None is passed as a NULL pointer.  -> (counts (H,), transforms (H,4,4))."""
    import torch
    from catgrasp_amd import _lib as L
    ids = np.ascontiguousarray(ids, dtype=np.int32).reshape(-1, 4)
    counts = torch.full((len(ids),), -7, dtype=torch.int32, device=dev)
    Ts = torch.full((len(ids), 16), -7.0, dtype=torch.float64, device=dev)
    D3 = ctypes.c_double * 3
    d_src, d_dst, d_ids = _d(src, dev), _d(dst, dev), _d(ids, dev)
    L.check(L.lib().cg_ransac_9d(L._p(d_src), L._p(d_dst), len(src), L._p(d_ids), len(ids), float(thres),
                                 D3(*[float(v) for v in min_s]), D3(*[float(v) for v in max_s]), None if max_d is None else D3(*[float(v) for v in max_d]),
                                 L._p(counts), L._p(Ts), L._stream()), 'cg_ransac_9d')
    return counts.cpu().numpy(), Ts.cpu().numpy().reshape(-1, 4, 4)


def _inlier_mask(dev, src, dst, T, thres):
    import torch
    from catgrasp_amd import _lib as L
    mask = torch.full((len(src),), 7, dtype=torch.uint8, device=dev)
    d_src, d_dst, d_T = _d(src, dev), _d(dst, dev), _d(np.asarray(T, dtype=np.float64).reshape(16), dev)
    L.check(L.lib().cg_similarity_inliers(L._p(d_src), L._p(d_dst), len(src), L._p(d_T), float(thres), L._p(mask), L._stream()), 'cg_similarity_inliers')
    return mask.cpu().numpy()


@pytest.mark.parametrize('dims', G.RANSAC_DIMS)
@pytest.mark.parametrize('n', G.RANSAC_N)
def test_ransac_gates_and_counts_match_the_oracle(cuda_device, n, dims):
    """400 hypotheses on N points around the wave (64) and block (256) widths, with the extent gate off, loose and tight: accept /
    reject and inlier count of every hypothesis, every accepted transform, the winner's inlier mask and the wrapper's answer.
    Hypotheses within 1e-9 of a gate threshold in the oracle may be left out (Jacobi against LAPACK); at most 1 % are."""
    from catgrasp_amd import aligning
    c = G.ransac_case(n, dims)
    keep = ~c['near']
    print(f'N = {n}, max_dimensions = {dims}: {int((~keep).sum())} of {len(keep)} hypotheses left out')
    assert (~keep).mean() <= 0.01
    counts, Ts = _ransac(cuda_device, c['src'], c['dst'], c['ids'], G.RANSAC_THRES, G.MIN_SCALE, G.MAX_SCALE, c['max_d'])
    assert np.array_equal(counts[keep], c['ref_counts'][keep]), f'{(counts != c["ref_counts"])[keep].sum()} hypotheses disagree'
    assert np.abs(Ts[keep] - c['ref_T'][keep]).max() < 1e-9                              # rejected ones are all zero on both sides
    acc = np.flatnonzero(c['ref_counts'] >= 0)
    best = acc[np.argmax(c['ref_counts'][acc])]                                          # the first maximum
    assert keep[best]
    mask = _inlier_mask(cuda_device, c['src'], c['dst'], Ts[best], G.RANSAC_THRES)
    assert np.array_equal(np.flatnonzero(mask), c['inl_ref']) and set(np.unique(mask)) <= {0, 1}
    T, inl = aligning.estimate9DTransform(c['src'], c['dst'], G.RANSAC_THRES, max_iter=len(c['ids']), max_scale=G.MAX_SCALE, min_scale=G.MIN_SCALE,
                                          max_dimensions=c['max_d'], ids=c['ids'], device=cuda_device)
    assert np.abs(T - c['T_ref']).max() < 1e-9 and np.array_equal(inl, c['inl_ref'])


def test_ransac_exact_tetrahedron(cuda_device):
    """Residuals of exactly thres count, 2^-40 more does not; a scale of exactly max_scale = min_scale passes, 2^-40 less room rejects."""
    src, dst = G.tetra_problem()
    two = np.array([2.0, 2.0, 2.0])
    T = np.eye(4); T[:3, :3] *= 2; T[:3, 3] = G.TETRA_T
    ids = np.array([[0, 1, 2, 3]])
    for thres, cnt, mask in ((0.25, 6, [1, 1, 1, 1, 1, 0, 1]), (0.25 - 2.0 ** -40, 4, [1, 1, 1, 1, 0, 0, 0])):
        counts, Ts = _ransac(cuda_device, src, dst, ids, thres, two, two, None)
        assert counts.tolist() == [cnt]
        assert np.array_equal(Ts[0].view(np.uint64), T.view(np.uint64))
        assert _inlier_mask(cuda_device, src, dst, T, thres).tolist() == mask
    counts, Ts = _ransac(cuda_device, src, dst, ids, 0.25, two, two - 2.0 ** -40, None)
    assert counts.tolist() == [-1] and not Ts.any()
    counts, _ = _ransac(cuda_device, src, dst, ids, 0.25, two + 2.0 ** -40, two + 1, None)
    assert counts.tolist() == [-1]


def test_ransac_four_points_one_hypothesis(cuda_device):
    src, dst, ids = G.four_point_problem()
    for dims in G.RANSAC_DIMS:
        max_d = None if dims is None else np.array([dims] * 3)
        T_ref, inl_ref, outs = aligning_ref.estimate9DTransform(src, dst, G.RANSAC_THRES, ids, G.MAX_SCALE, G.MIN_SCALE, max_d)
        counts, Ts = _ransac(cuda_device, src, dst, ids, G.RANSAC_THRES, G.MIN_SCALE, G.MAX_SCALE, max_d)
        assert outs[0][0] == 4 and counts.tolist() == [4]
        assert np.abs(Ts[0] - T_ref).max() < 1e-9


def test_ransac_mirrored_source_is_rejected_by_the_determinant(cuda_device):
    from catgrasp_amd import aligning
    c = G.ransac_case(63, None)
    src = c['src'] * np.array([-1.0, 1.0, 1.0])
    ids = c['ids'][:200]
    counts, Ts = _ransac(cuda_device, src, c['dst'], ids, G.RANSAC_THRES, G.MIN_SCALE, G.MAX_SCALE, None)
    assert (counts == -1).all() and not Ts.any()
    assert aligning.estimate9DTransform(src, c['dst'], G.RANSAC_THRES, max_iter=200, max_scale=G.MAX_SCALE, min_scale=G.MIN_SCALE, ids=ids,
                                        device=cuda_device) == (None, None)


def test_ransac_degenerate_samples_are_rejected(cuda_device):
    """Exactly coplanar, exactly collinear and repeated samples have no affine model; a proper sample of the same cloud has."""
    src, dst, ids = G.degenerate_problem()
    ids = np.concatenate([ids, [[0, 1, 2, 6]]])
    counts, Ts = _ransac(cuda_device, src, dst, ids, 0.25, [0.0] * 3, [99.0] * 3, None)
    assert counts.tolist() == [-1, -1, -1, len(src)] and not Ts[:3].any()
