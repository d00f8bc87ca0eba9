"""Plain float64 restatements of the grasp-geometry kernels (csrc/affordance.hip, conesampler.hip, ransac.hip) and the scenes
their edge tests run on.  No kd-tree, and no LAPACK on anything that is compared bit for bit: every value below is a fixed sequence
of IEEE double products, sums and one division, so on exact-arithmetic inputs (dyadic lattice coordinates, signed-permutation
rotations) it equals the kernel in every bit whatever order the kernel sums in.

test_geometry_ref_cpu.py pins these restatements against the oracles (oracle/affordance_ref.py, grasp_sampler_ref.py,
aligning_ref.py) and asserts that the scenes reach the edges they are built for; test_geometry_edges_gpu.py runs the kernels."""
import functools
import itertools

import numpy as np

from catgrasp_amd import synth
from oracle import aligning_ref

NAN = float('nan')


def _rows(T12, p):
    """q = [R|t] p for every row of p, summed left to right like the kernels."""
    T = np.asarray(T12, dtype=np.float64).reshape(-1)[:12]
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    return [T[4 * i] * x + T[4 * i + 1] * y + T[4 * i + 2] * z + T[4 * i + 3] for i in range(3)]


def finger_patch_detail(T12, pts, nrm, aff, extent4, grip_sign, tol):
    """One finger of cg_grasp_affordance, with what the edge census needs.  -> dict(count, mean, within, d, patch, first, dot)."""
    T = np.asarray(T12, dtype=np.float64).reshape(-1)
    qx, qy, qz = _rows(T, pts)
    xmin, xmax, zmin, zmax = extent4
    within = (qx >= xmin) & (qx <= xmax) & (qz >= zmin) & (qz <= zmax)
    out = dict(count=0, mean=None, within=within, qx=qx, qz=qz, d=None, patch=None, first=None, dot=None)
    if not within.any():
        return out
    yref = qy[within].min() if grip_sign > 0 else qy[within].max()      # the first point the closing finger touches
    d = np.abs(qy - yref)
    patch = within & (d <= tol)
    ids = np.flatnonzero(patch)
    first = int(ids[np.argmin(d[ids])])                                 # first index realising the minimum distance
    n = nrm[first]
    dot = (T[4] * n[0] + T[5] * n[1] + T[6] * n[2]) * float(grip_sign)
    out.update(d=d, patch=patch, first=first, dot=dot)
    if dot > 0.0:                                                        # that point's normal faces along grip_dir: no contact
        return out
    s = 0.0
    for i in ids:
        s += float(aff[i])
    out.update(count=len(ids), mean=s / len(ids))
    return out


def finger_patch(T12, pts, nrm, aff, extent4, grip_sign, tol):
    """-> (count, mean affordance over the contact patch or None)."""
    r = finger_patch_detail(T12, pts, nrm, aff, extent4, grip_sign, tol)
    return r['count'], r['mean']


def p_t_given_g(T12, pts, nrm, aff, extents, grip_signs, tol):
    """-> (mean over the fingers that have a patch, NaN if none; per-finger counts)."""
    acc, nvalid, counts = 0.0, 0, []
    for e, s in zip(extents, grip_signs):
        c, m = finger_patch(T12, pts, nrm, aff, e, s, tol)
        counts.append(c)
        if m is not None:
            acc += m; nvalid += 1
    return (acc / nvalid if nvalid else NAN), counts


def nearest_first(query, ref, chunk=2048):
    """argmin_r (dx*dx + dy*dy) + dz*dz with d = ref_r - query, first minimum.  -> (Q,) int32."""
    query = np.asarray(query, dtype=np.float64).reshape(-1, 3); ref = np.asarray(ref, dtype=np.float64).reshape(-1, 3)
    out = np.empty(len(query), dtype=np.int32)
    for a in range(0, len(query), chunk):
        q = query[a:a + chunk]
        dx = ref[None, :, 0] - q[:, None, 0]; dy = ref[None, :, 1] - q[:, None, 1]; dz = ref[None, :, 2] - q[:, None, 2]
        out[a:a + chunk] = np.argmin(dx * dx + dy * dy + dz * dz, axis=1)
    return out


def center_y(poses, pts):
    """cg_center_grasps: every pose shifted along its own y axis to the middle of the cloud's y extent in the pose's frame."""
    out = np.array(poses, dtype=np.float64).reshape(-1, 4, 4).copy()
    x, y, z = pts[:, 0], pts[:, 1], pts[:, 2]
    for T in out:
        r0, r1, r2 = T[0, 1], T[1, 1], T[2, 1]
        ty = -(r0 * T[0, 3] + r1 * T[1, 3] + r2 * T[2, 3])
        v = r0 * x + r1 * y + r2 * z + ty
        cy = (v.max() + v.min()) / 2
        for i in range(3):
            T[i, 3] += T[i, 1] * cy
    return out


def similarity_residuals(src, dst, T):
    T = np.asarray(T, dtype=np.float64).reshape(-1)
    e2 = 0.0
    for i, q in enumerate(_rows(T, src)):
        c = q - dst[:, i]
        e2 = e2 + c * c
    return np.sqrt(e2)


def similarity_inliers(src, dst, T, thres):
    """cg_similarity_inliers: |T src - dst| <= thres.  -> (N,) uint8."""
    return (similarity_residuals(src, dst, T) <= thres).astype(np.uint8)


# ------------------------------------------------------------------------------------------------------------------------------
# the lattice scene of the affordance kernel: every coordinate a multiple of 1/64, every rotation a signed permutation

def signed_permutations():
    """The 24 proper rotations whose entries are 0 and +-1."""
    out = []
    for perm in itertools.permutations(range(3)):
        for sg in itertools.product((1.0, -1.0), repeat=3):
            R = np.zeros((3, 3))
            for i in range(3):
                R[i, perm[i]] = sg[i]
            if np.linalg.det(R) > 0:
                out.append(R)
    assert len(out) == 24
    return out


LATTICE_EXTENT = (-0.25, 0.25, -0.125, 0.375)       # finger box: x range, z range
LATTICE_TOL = 1.0 / 32


@functools.lru_cache(maxsize=None)
def lattice_scene():
    """-> dict(pts (130,3), nrm (130,3), aff (130,), T (480,12) rows [R|t])."""
    rng = np.random.default_rng(20)
    pts = rng.integers(-32, 33, (130, 3)) / 64.0
    nrm = rng.integers(-2, 3, (130, 3)).astype(np.float64)
    aff = rng.integers(0, 1025, 130) / 1024.0
    trans = rng.integers(-16, 17, (20, 3)) / 64.0
    T = np.array([np.concatenate([R, t.reshape(3, 1)], axis=1).reshape(12) for R in signed_permutations() for t in trans])
    return dict(pts=pts, nrm=nrm, aff=aff, T=T)


def to44(T12):
    T = np.eye(4); T[:3] = np.asarray(T12).reshape(3, 4)
    return T


def tie_scene(gap, swapped):
    """Two points at the same place are both the first the +y finger touches (distance exactly 0): index 3 and index 3 + gap.  One
    normal faces along grip_dir (a finger that touches it first has no contact), the other against it; `swapped` puts the accepting
    one first.  gap = 64 puts both in one lane of the wave, gap = 1 in neighbouring lanes.  Every other point lies strictly behind."""
    s = lattice_scene()
    pts, nrm = s['pts'].copy(), s['nrm'].copy()
    pts[:, 1] = np.maximum(pts[:, 1], -0.5 + 1.0 / 64)
    for i, n in ((3, (0.0, 1.0, 0.0)), (3 + gap, (0.0, -1.0, 0.0))):
        pts[i] = (0.0, -0.5, 0.0); nrm[i] = n
    if swapped:
        nrm[[3, 3 + gap]] = nrm[[3 + gap, 3]]
    return pts, nrm, s['aff'], np.eye(4)[:3].reshape(12)


def random_affordance_scene(P=65, n_poses=400):
    """The scene of tests/test_affordance_gpu.py, down-sampled to P points."""
    rng = np.random.default_rng(0)
    ob = synth.make_scene(1, 6000, 3)[0]
    aff = rng.uniform(0, 1, P)
    sel = rng.choice(len(ob['xyz']), P, replace=False)
    pts, nrm = ob['xyz'][sel] + rng.normal(0, 2e-5, (P, 3)), ob['normal'][sel]
    g = synth.make_gripper()
    return pts, nrm, aff, [g['vertices'][8:16], g['vertices'][16:24]], g['gripper_in_grasp'], synth.make_candidates(ob, n_poses, rng)


# ------------------------------------------------------------------------------------------------------------------------------
# RANSAC problems and the gate census

RANSAC_N = (63, 64, 65, 255, 256, 257, 700)
RANSAC_DIMS = (None, 1.2, 1.02)
RANSAC_H = 400
RANSAC_THRES = 0.003
MIN_SCALE, MAX_SCALE = (0.005, 0.005, 0.001), (0.05, 0.05, 0.05)
NEAR = 1e-9                      # a hypothesis this close (relative) to a gate threshold may differ between Jacobi and LAPACK


def ransac_problem(seed, n, outliers=0.15, noise=1e-4):
    """tests/test_aligning_gpu.py::_problem: NUNOCS predictions of a posed, anisotropically scaled cloud, some of them wrong."""
    rng = np.random.default_rng(seed)
    nocs = rng.uniform(-0.5, 0.5, (n, 3))
    R = synth.random_rotation(rng); s = np.array([0.016, 0.02, 0.007]); t = np.array([0.02, -0.03, 0.62])
    T = np.eye(4); T[:3, :3] = R @ np.diag(s); T[:3, 3] = t
    obs = nocs @ T[:3, :3].T + t + rng.normal(0, noise, (n, 3))
    bad = rng.random(n) < outliers
    nocs_pred = nocs.copy()
    nocs_pred[bad] = rng.uniform(-0.5, 0.5, (bad.sum(), 3))
    return nocs_pred, obs, T


def ransac_gates(src, dst, ids, thres, min_scale, max_scale, max_dims):
    """The oracle's worker (oracle/aligning_ref.py) walked gate by gate.  -> (stage (H,) of '' (accepted), 'degenerate', 'scale',
    'sv', 'det', 'extent'; near (H,) bool: some quantity the hypothesis reached lies within NEAR of its threshold)."""
    stage, near = [], []
    mn, mx = np.asarray(min_scale, dtype=np.float64), np.asarray(max_scale, dtype=np.float64)

    def close(v, thr):
        return bool(np.any(np.abs(np.asarray(v) - thr) <= NEAR * np.abs(thr)))

    for row in ids:
        s4, d4 = src[row], dst[row]
        M = np.concatenate([s4, np.ones((4, 1))], axis=1)
        cut = 1e-13 * max(np.abs(s4).max(), 1e-300) ** 3
        nr = close(abs(np.linalg.det(M)), cut)
        T = aligning_ref.affine_from_4(s4, d4)
        if T is None:
            stage.append('degenerate'); near.append(nr); continue
        sc = np.linalg.norm(T[:3, :3], axis=0)
        nr |= close(sc, mn) or close(sc, mx)
        if (sc > mx).any() or (sc < mn).any() or not (sc > 0).all():
            stage.append('scale'); near.append(nr); continue
        u, sv, vh = np.linalg.svd(T[:3, :3] / sc.reshape(1, 3))
        nr |= close(sv.min(), 0.8) or close(sv.max(), 1.2)
        if sv.min() < 0.8 or sv.max() > 1.2:
            stage.append('sv'); near.append(nr); continue
        R = u @ vh
        if np.linalg.det(R) < 0:
            stage.append('det'); near.append(nr); continue
        new_t = T.copy(); new_t[:3, :3] = R @ np.diag(sc)
        if max_dims is not None:
            can = (np.linalg.inv(new_t) @ np.concatenate([dst, np.ones((len(dst), 1))], 1).T).T[:, :3]
            ext = can.max(axis=0) - can.min(axis=0)
            nr |= close(ext, np.asarray(max_dims, dtype=np.float64))
            if (ext > max_dims).any():
                stage.append('extent'); near.append(nr); continue
        st = (new_t @ np.concatenate([src, np.ones((len(src), 1))], 1).T).T[:, :3]
        nr |= close(np.linalg.norm(st - dst, axis=-1), thres)
        stage.append(''); near.append(nr)
    return np.array(stage), np.array(near, dtype=bool)


@functools.lru_cache(maxsize=None)
def ransac_case(n, dims):
    """One census case, evaluated once by the oracle.  -> dict(src, dst, ids, max_d, T_ref, inl_ref, ref_counts, ref_T, stage, near)."""
    src, dst, _ = ransac_problem(100 + n, n)
    rng = np.random.default_rng(n)
    ids = np.stack([rng.choice(n, 4, replace=False) for _ in range(RANSAC_H)]).astype(np.int32)
    max_d = None if dims is None else np.array([dims] * 3)
    T_ref, inl_ref, outs = aligning_ref.estimate9DTransform(src, dst, RANSAC_THRES, ids, MAX_SCALE, MIN_SCALE, max_d)
    stage, near = ransac_gates(src, dst, ids, RANSAC_THRES, MIN_SCALE, MAX_SCALE, max_d)
    ref_counts = np.array([-1 if o is None else o[0] for o in outs])
    ref_T = np.array([np.zeros((4, 4)) if o is None else o[1] for o in outs])
    return dict(src=src, dst=dst, ids=ids, max_d=max_d, T_ref=T_ref, inl_ref=inl_ref, ref_counts=ref_counts, ref_T=ref_T, stage=stage,
                near=near)


def four_point_problem():
    """N = 4, the smallest cloud the kernel takes: its one possible sample is the whole cloud (seed 0 is the first whose sample the
    oracle accepts)."""
    src, dst, _ = ransac_problem(0, 4)
    return src, dst, np.array([[0, 1, 2, 3]], dtype=np.int32)


TETRA_T = (0.5, -0.25, 2.0)


def tetra_problem():
    """The unit tetrahedron doubled and shifted: every number a small dyadic, so elimination, scales, Jacobi (nothing to rotate) and
    residuals are exact.  Points 4..6 miss their targets by exactly 0.25, 0.25 + 2^-40 and 0.25.  Points 7.. only serve the
    degenerate samples.  -> (src, dst)."""
    src = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [0.5, 0.25, -1], [-0.75, 2, 0.5], [1.5, -0.5, 0.125]], dtype=np.float64)
    dst = 2.0 * src + np.array(TETRA_T)
    dst[4, 0] += 0.25
    dst[5, 1] += 0.25 + 2.0 ** -40
    dst[6, 2] -= 0.25
    return src, dst


def degenerate_problem():
    """Lattice points with exactly coplanar and exactly collinear quadruples.  -> (src, dst, ids (3,4): coplanar, collinear, repeated)."""
    src = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0], [2, 0, 0], [4, 0, 0], [0, 0, 1], [0.5, 0.25, -1]], dtype=np.float64)
    dst = 2.0 * src + np.array(TETRA_T)
    ids = np.array([[0, 1, 2, 3], [0, 1, 4, 5], [0, 0, 1, 6]], dtype=np.int32)
    return src, dst, ids


# ------------------------------------------------------------------------------------------------------------------------------
# the built cloud of the cone sampler

CONE_R = 1.0 / 64
CONE_KW = dict(hand_depth=0.04, init_bite=0.005, approach_step=0.015)
CONE_STEP_DEG = 50.0                                # 180 / 50 is no integer: np.arange(0, 180, 50) has 4 entries
CONE_SPHERE = np.array([[1.0, 0, 0], [-1.0, 0, 0], [0, 0, 1.0], [-1.0, 2.0 ** -20, 0]])


def cone_cloud(P):
    """-> (pts (P,3), nrm (P,3), sample ids in walking order).  With r = CONE_R:
    cluster A around point 0: three neighbours at exactly r, a duplicate of point 0 (distance 0: not a neighbour), a closer point with
    a zero normal (ignored);
    cluster B around point 7: its only neighbour inside r has normal (1,-1,0), whose n n^T sums to exactly 0, so the radius doubles
    -- for good, like the reference's -- and at 2r a point at exactly 2r ends the doubling.
    Far-away filler points bring the cloud to P points.  P = 2 is point 0 and one neighbour at exactly r."""
    u = CONE_R
    if P == 2:
        return np.array([[0, 0, 0], [u, 0, 0]]), np.array([[0, 0, 1.0], [0, 3.0, 0]]), np.array([0], dtype=np.int32)
    base = [((0, 0, 0), (0, 0, 1)),                 # 0  sample
            ((u, 0, 0), (2, 1, 0)),                 # 1  at exactly r
            ((0, -u, 0), (0, 1, 3)),                # 2  at exactly r
            ((0, 0, u), (1, 0, 1)),                 # 3  at exactly r
            ((0, 0, 0), (5, 0, 0)),                 # 4  duplicate of the sample point
            ((u / 2, u / 2, 0), (0, 0, 0)),         # 5  inside, zero normal
            ((u / 2, 0, u / 4), (1, 1, 1)),         # 6  inside
            ((1, 0, 0), (0, 1, 0)),                 # 7  sample of cluster B
            ((1 + u / 2, 0, 0), (1, -1, 0)),        # 8  the only point within r of 7
            ((1, 2 * u, 0), (0, 0, 3))]             # 9  at exactly 2r of 7
    pts = np.array([b[0] for b in base], dtype=np.float64); nrm = np.array([b[1] for b in base], dtype=np.float64)
    assert P >= len(base)
    k = np.arange(P - len(base), dtype=np.float64)
    pts = np.concatenate([pts, np.stack([4 + k, 3 + 0 * k, 1 + 0 * k], axis=1)])
    nrm = np.concatenate([nrm, np.tile([0.0, 0, 1], (len(k), 1))])
    return pts, nrm, np.array([0, 7, 0, 1, 9], dtype=np.int32)
