"""Host references of the input-building and SDF kernels (cg_build_grasp_input, cg_build_nunocs_input, cg_softmax_pg,
cg_sdf_points_inside_batch), their derived error bounds and the seeded inputs of their tests.

Used by tests/test_prep_kernels_gpu.py and tests/test_sdf_gpu.py, and proved on the CPU by tests/test_prep_ref_cpu.py.

The library is compiled with -ffp-contract=off and without fast-math, so every product, sum, fmaf and division of these kernels is
one correctly rounded float32 operation and the whole chain can be restated here bit for bit (numpy's float32 +, -, *, / are
correctly rounded; dense_ref.fmaf is the correctly rounded fused multiply-add).  Only cg_softmax_pg cannot: the device expf is
not correctly rounded, so its probabilities are held to a measured bound (see test_prep_kernels_gpu.py).

Rounding model of the bounds (u = 2^-24, gamma_n = n u / (1 - n u), as tests/dense_ref.py):
  * transform chains  y = T p + t  evaluated as three nested fmaf on float32 roundings of T, p and t:
        |y^ - y| <= (gamma_4 + 2u) (|T| |p| + |t|)
    the chain itself rounds three times (gamma_3 on the magnitudes of the rounded inputs), rounding T and the point to float32
    moves every product by at most (2u + u^2) of its magnitude and t by u; the fourth u of gamma_4 covers the second-order terms.
    The float64 references invert a rigid 4x4 pose; F64 below covers their own rounding.
  * the normaliser  (v - mean) * inv_std  as two rounded operations on float32 roundings of mean and 1 / (std + 1e-15): with
    a = y - mean the exact difference and e_v the bound on v,
        e_a   = e_v + u |mean| + u (|a| + e_v + u |mean|)                    (input error, mean's rounding, the subtraction)
        e_out = s (e_a + gamma_3 (|a| + e_a)),  s = 1 / (std + 1e-15)        (inv_std's rounding, the product's; one u spare)
  * NormalizeCloud: minimum and maximum are exact selections and rounding to float32 is monotone, so min^ = fl(min); see
    nunocs_bound for the quotient.
Underflow: every operation may also err by half the smallest subnormal; TINY is added once per bound.
"""
import numpy as np

import dense_ref as R
from catgrasp_amd import synth
from oracle import sdf_ref
from oracle import transforms_ref as tref

f32 = np.float32
U32 = R.U32
gamma = R.gamma
fmaf = R.fmaf
F64 = 64 * 2.0 ** -53          # relative error allowed to a float64 reference (inverse of a rigid pose, a 4-term dot product)
TINY = 8 * 2.0 ** -150         # a few float32 operations' underflow
BGI_CPB, BGI_CAP = 8, 2688     # csrc/misc.hip: candidates per workgroup and points of the LDS slice


# ----------------------------------------------------------------------------------------------------------- normaliser
def normalise_chain(v, mean, inv_std, fused=False):
    """(v - mean) * inv_std, two rounded float32 operations (both kernels).  fused: planted defect, v * inv_std - mean * inv_std
    in one fused operation."""
    if mean is None:
        return v
    m = np.asarray(mean, f32)
    s = np.asarray(inv_std, f32)
    if fused:
        return fmaf(v, s, -(m * s))
    return ((v - m).astype(f32) * s).astype(f32)


def normalise_bound(ref, e_v, mean, std):
    """Bound of the normalised value from the bound e_v of the plain one.  ref: the float64 NORMALISED reference,
    (y - mean) / (std + 1e-15), from which |a| = |y - mean| is recovered."""
    mean = np.asarray(mean, np.float64)
    s = 1.0 / (np.asarray(std, np.float64) + 1e-15)
    a = np.abs(ref) / s
    e_a = e_v + U32 * np.abs(mean) + U32 * (a + e_v + U32 * np.abs(mean))
    return s * (e_a + gamma(3) * (a + e_a)) + TINY


# ----------------------------------------------------------------------------------------------------- build_grasp_input
def grasp_chain_points(T12, p, n, mean=None, inv_std=None, normal_plus_t=False, fused_norm=False):
    """grasp_point of csrc/misc.hip on gathered points: T12 (G,12), p / n (G,n_pts,3) float32 -> (G,n_pts,6) float32.
    normal_plus_t / fused_norm: planted defects (the normal chain with the translation added; a fused normaliser)."""
    T = np.asarray(T12, f32)[:, None, :]
    p = np.asarray(p, f32)
    n = np.asarray(n, f32)
    out = np.empty(p.shape[:2] + (6,), f32)
    for j in range(3):
        t0, t1, t2, t3 = (T[..., 4 * j + k] for k in range(4))
        out[..., j] = fmaf(t0, p[..., 0], fmaf(t1, p[..., 1], fmaf(t2, p[..., 2], t3)))
        tail = fmaf(t2, n[..., 2], t3) if normal_plus_t else (t2 * n[..., 2]).astype(f32)
        out[..., 3 + j] = fmaf(t0, n[..., 0], fmaf(t1, n[..., 1], tail))
    return normalise_chain(out, mean, inv_std, fused=fused_norm)


def grasp_point_chain(T12, xyz, nrm, ids, mean=None, inv_std=None):
    """cg_build_grasp_input bit for bit: gather, then the chain of grasp_point."""
    ids = np.asarray(ids)
    return grasp_chain_points(T12, np.asarray(xyz, f32)[ids], np.asarray(nrm, f32)[ids], mean, inv_std)


def staged_gather(xyz, nrm, ids, n_cloud, defect=None):
    """The point selection of build_grasp_input_staged_kernel: per workgroup of BGI_CPB candidates, the slice [cur_lo, cur_hi] kept
    across candidates, re-staged when a candidate's id range leaves it, gathers from global memory when the range exceeds BGI_CAP.
    -> (p, n, trace): the points every candidate reads, (G,n_pts,3) each, and per candidate a dict(path 'stage' | 'reuse' |
    'global', lo, hi, cur_lo, tail: the copy's scalar tail runs).
    defect: 'off_by_one' (the slice is indexed one point too far), 'no_granule' (the slice is copied from the 4-point granule
    lo & ~3 but indexed as if it started at lo)."""
    xyz = np.asarray(xyz, f32)
    nrm = np.asarray(nrm, f32)
    ids = np.asarray(ids)
    G = len(ids)
    p = np.empty(ids.shape + (3,), f32)
    n = np.empty(ids.shape + (3,), f32)
    trace = []
    for g in range(G):
        if g % BGI_CPB == 0:
            cur_lo, cur_hi, base = 0, -1, 0
            sx = sn = None
        lo, hi = int(ids[g].min()), int(ids[g].max())
        staged = lo >= cur_lo and hi <= cur_hi
        path = 'reuse' if staged else 'global'
        tail = False
        if not staged and lo >= 0 and hi < n_cloud and hi - (lo & ~3) + 1 <= BGI_CAP:
            cur_lo, cur_hi = lo & ~3, hi
            base = lo if defect == 'no_granule' else cur_lo
            sx, sn = xyz[cur_lo:cur_hi + 1].copy(), nrm[cur_lo:cur_hi + 1].copy()
            tail = ((cur_hi - cur_lo + 1) * 3) % 4 != 0
            staged, path = True, 'stage'
        if staged:
            k = ids[g] - base + (1 if defect == 'off_by_one' else 0)
            k = np.clip(k, 0, len(sx) - 1)              # the defective variants stay inside the emulated LDS array
            p[g], n[g] = sx[k], sn[k]
        else:
            p[g], n[g] = xyz[ids[g]], nrm[ids[g]]
        trace.append({'path': path, 'lo': lo, 'hi': hi, 'cur_lo': cur_lo, 'tail': tail})
    return p, n, trace


def grasp_ref64(case):
    """transforms_ref.grasp_transform per candidate on the float64 scene cloud -> (G,n_pts,6) float64."""
    return np.stack([tref.grasp_transform(case['xyz64'].copy(), case['nrm64'].copy(), case['poses'][g], case['ids'][g],
                                          case['mean64'], case['std64'])['input'] for g in range(len(case['poses']))])


def grasp_bound(case, ref):
    """Bound (G,n_pts,6) on |cg_build_grasp_input - grasp_ref64|: (gamma_4 + 2u)(|T| |p| + |t|) on the centred cloud the kernel
    reads (T p_c + t' = T p + t exactly), propagated through the normaliser when there is one."""
    aT = np.abs(case['T12'].astype(np.float64))[:, None, :]
    ap = np.abs(case['xyz32'].astype(np.float64))[case['ids']]
    an = np.abs(case['nrm32'].astype(np.float64))[case['ids']]
    mag = np.empty(ap.shape[:2] + (6,))
    for j in range(3):
        mag[..., j] = aT[..., 4 * j] * ap[..., 0] + aT[..., 4 * j + 1] * ap[..., 1] + aT[..., 4 * j + 2] * ap[..., 2] + aT[..., 4 * j + 3]
        mag[..., 3 + j] = aT[..., 4 * j] * an[..., 0] + aT[..., 4 * j + 1] * an[..., 1] + aT[..., 4 * j + 2] * an[..., 2]
    # the float64 reference works on the uncentred cloud: its own rounding is relative to those larger magnitudes
    m64 = 3 * np.abs(case['xyz64']).max() + np.abs(np.linalg.inv(case['poses'])[:, :3, 3]).max(axis=1)
    e = (gamma(4) + 2 * U32) * mag + F64 * m64[:, None, None] + TINY
    if case['mean64'] is None:
        return e
    return normalise_bound(ref, e, case['mean64'], case['std64'])


def check_grasp(case, out, what):
    """The comparison of the GPU tests: bit for bit against the float32 chain, and within the derived bound of float64.
    -> worst error / bound ratio."""
    R.check_bitwise(out, grasp_point_chain(case['T12'], case['xyz32'], case['nrm32'], case['ids'], case['mean32'], case['inv_std32']),
                    what + ' vs the float32 chain')
    ref = grasp_ref64(case)
    return R.check_bound(out, ref, grasp_bound(case, ref), what + ' vs float64')


def _normaliser(rng, with_mean):
    if not with_mean:
        return None, None, None, None
    mean = rng.normal(0, 0.002, 6)
    std = rng.uniform(0.004, 0.3, 6)
    return mean, std, mean.astype(f32), (1.0 / (std + 1e-15)).astype(f32)


def _object(n, seed):
    return synth.make_scene(1, n, seed=seed)[0]


def _scene_case(sizes, obj_of_g, n_pts, seed, with_mean, draw=None):
    """A concatenated scene of len(sizes) objects (as SceneBatch lays them out), candidate g on object obj_of_g[g] with ids inside
    that object's slice, the cloud centred and rounded once as transforms.DeviceCloud does, T12 as transforms.pose_inverse_rows.
    draw(rng, g, k, n) -> local ids of candidate g (default: a numpy choice that always holds the object's first and last point,
    so the staged range of an object is its whole slice)."""
    from catgrasp_amd import transforms
    rng = np.random.default_rng(seed)
    objs = [_object(n, 100 * seed + k) for k, n in enumerate(sizes)]
    base = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)
    xyz64 = np.concatenate([o['xyz'] for o in objs])
    nrm64 = np.concatenate([o['normal'] for o in objs])
    center = xyz64.mean(axis=0)
    poses, ids = [], []
    for g, k in enumerate(obj_of_g):
        poses.append(synth.make_candidates(objs[k], 1, rng)[0])
        if draw is not None:
            loc = draw(rng, g, k, sizes[k])
        else:
            loc = rng.choice(sizes[k], n_pts, replace=sizes[k] < n_pts)
            loc[rng.integers(0, n_pts // 2)] = 0
            loc[n_pts // 2 + rng.integers(0, n_pts - n_pts // 2)] = sizes[k] - 1
        ids.append(base[k] + loc)
    poses = np.array(poses)
    mean64, std64, mean32, inv_std32 = _normaliser(rng, with_mean)
    return {'xyz64': xyz64, 'nrm64': nrm64, 'xyz32': (xyz64 - center).astype(f32), 'nrm32': nrm64.astype(f32), 'poses': poses,
            'T12': transforms.pose_inverse_rows(poses, center), 'ids': np.array(ids).astype(np.int32), 'base': base, 'sizes': list(sizes),
            'obj_of_g': list(obj_of_g), 'mean64': mean64, 'std64': std64, 'mean32': mean32, 'inv_std32': inv_std32}


def grasp_case(name):
    """The seeded inputs of the build_grasp_input cases (module docstring of test_prep_kernels_gpu.py)."""
    if name == 'S1':            # one object that fits the slice, 20 candidates = 2 1/2 workgroups, 2048 points each
        def draw(rng, g, k, n):
            loc = rng.choice(n, 2048, replace=False)
            if g % BGI_CPB == 0:                       # a workgroup's first candidate stages the whole object: the others reuse it
                loc[:2] = (0, n - 1)
            return loc
        return _scene_case([2500], [0] * 20, 2048, 11, True, draw)
    if name == 'S2':            # three objects: 1001 points (3003 floats: copy tail), bases 1001 (% 4 = 1) and 2503 (% 4 = 3)
        order = [0, 0, 0, 1, 1, 1, 1, 1, 1, 2, 2, 0, 0, 2, 2, 1, 1, 1, 0]
        return _scene_case([1001, 1502, 2000], order, 1024, 12, True)
    if name == 'S3':            # a 4000-point object between two that fit: staged, global, staged inside one workgroup
        sizes = [1500, 4000, 2000]
        order = [0, 0, 1, 0, 2, 1, 2, 0, 1, 0, 1, 1, 1, 2]
        # candidates 11 and 12 sit on the capacity test: their ranges are exactly BGI_CAP points (staged) and BGI_CAP + 1 (global)
        width = {11: BGI_CAP, 12: BGI_CAP + 1}

        def draw(rng, g, k, n):
            if g in width:
                w = width[g]
                loc = 100 + rng.choice(w, 1024, replace=False)        # base 1500 + 100 = 1600, a multiple of 4: lo & ~3 = lo
                loc[:2] = (100, 100 + w - 1)
                return loc
            loc = rng.choice(n, 1024, replace=False)
            loc[:2] = (0, n - 1)
            return loc
        return _scene_case(sizes, order, 1024, 13, True, draw)
    if name.startswith('S4-') or name[0] in 'PX':
        n_pts, G, with_mean = {'S4-64': (64, 9, True), 'S4-64-nomean': (64, 9, False), 'S4-128': (128, 9, True),
                               'S4-128-nomean': (128, 9, False), 'S4-1088': (1088, 9, True), 'S4-1088-nomean': (1088, 9, False),
                               'P1': (100, 5, True), 'P1-nomean': (100, 5, False), 'P2': (33, 4, True), 'P3': (33, 3, True),
                               'P4': (100, 5, True), 'X': (128, 9, True)}[name]
        return _scene_case([2500], [0] * G, n_pts, 14 + n_pts, with_mean, lambda rng, g, k, n: rng.choice(n, n_pts, replace=False))
    raise KeyError(name)


# ---------------------------------------------------------------------------------------------------- build_nunocs_input
def nunocs_input_chain(xyz, nrm, ids, mean=None, inv_std=None, no_eps=False):
    """cg_build_nunocs_input bit for bit: per cloud the per-axis min / max of the gathered points (exact, any order), scale = the
    largest of the three float32 extents, divisor scale + 1e-15f, (x - min) / divisor, normals copied, the normaliser.
    ids (B,n_pts) -> (B,n_pts,6) float32.  no_eps: planted defect, the divisor without + 1e-15f."""
    ids = np.asarray(ids)
    p = np.asarray(xyz, f32)[ids]
    lo, hi = p.min(axis=1), p.max(axis=1)
    scale = (hi - lo).astype(f32).max(axis=1)
    div = scale if no_eps else (scale + f32(1e-15)).astype(f32)
    with np.errstate(all='ignore'):
        q = ((p - lo[:, None, :]).astype(f32) / div[:, None, None]).astype(f32)
    return normalise_chain(np.concatenate([q, np.asarray(nrm, f32)[ids]], axis=-1), mean, inv_std)


def nunocs_ref64(case):
    """transforms_ref.normalize_cloud in float64 on the float64 cloud, normals alongside, the reference's normaliser."""
    out = []
    for ids in case['ids']:
        inp = np.concatenate([tref.normalize_cloud(case['xyz64'][ids]), case['nrm64'][ids]], axis=-1)
        if case['mean64'] is not None:
            inp = (inp - case['mean64'].reshape(1, -1)) / (case['std64'].reshape(1, -1) + 1e-15)
        out.append(inp)
    return np.stack(out)


def nunocs_bound(case, ref):
    """Bound (B,n_pts,6) on |cg_build_nunocs_input - nunocs_ref64|.  With x^ = fl(x) (|x^ - x| <= u |x|), l and h the float64 min
    and max of an axis (l^ = fl(l), h^ = fl(h)):
        numerator    fl(x^ - l^):        e_num = u (|x| + |l|) + u (|x - l| + u (|x| + |l|))
        extents      fl(h^ - l^):        e_ext = u (|h| + |l|) + u (|h - l| + u (|h| + |l|)), and max is 1-Lipschitz
        divisor      fl(scale^ + 1e-15f): e_div = max e_ext + u 1e-15 + u (d + max e_ext + 1e-15),  d = scale + 1e-15
        quotient     fl(num^ / div^):    e_q = (e_num + |q| e_div) / (d - e_div), then + u (|q| + e_q)
    which needs e_div < d: a degenerate cloud (extent 0, divisor 1e-15) has no float64 bound (inf here) and is held to the
    float32 chain's bytes alone.  Normals are copies of fl(n): u |n|."""
    with np.errstate(all='ignore'):
        e = np.empty(ref.shape)
        for b, ids in enumerate(case['ids']):
            x = np.abs(case['xyz64'][ids])
            pl, ph = case['xyz64'][ids].min(axis=0), case['xyz64'][ids].max(axis=0)
            l, h = np.abs(pl), np.abs(ph)
            e_num = U32 * (x + l) + U32 * (np.abs(case['xyz64'][ids] - pl) + U32 * (x + l))
            e_ext = (U32 * (h + l) + U32 * ((ph - pl) + U32 * (h + l))).max()
            d = (ph - pl).max() + 1e-15
            e_div = e_ext + U32 * 1e-15 + U32 * (d + e_ext + 1e-15)
            q = (case['xyz64'][ids] - pl) / d
            e_q = np.where(d > e_div, (e_num + q * e_div) / np.maximum(d - e_div, 1e-300), np.inf)
            e[b, :, :3] = e_q + U32 * (q + e_q) + TINY
            e[b, :, 3:] = U32 * np.abs(case['nrm64'][ids]) + TINY
        if case['mean64'] is None:
            return e
        return np.where(np.isfinite(e), normalise_bound(ref, np.where(np.isfinite(e), e, 0.0), case['mean64'], case['std64']), np.inf)


def check_nunocs(case, out, what):
    """-> worst error / bound ratio over the elements that have a finite bound."""
    R.check_bitwise(out, nunocs_input_chain(case['xyz32'], case['nrm32'], case['ids'], case['mean32'], case['inv_std32']),
                    what + ' vs the float32 chain')
    ref = nunocs_ref64(case)
    return R.check_bound(out, ref, nunocs_bound(case, ref), what + ' vs float64')


def nunocs_case(B, n_pts, with_mean, seed=0, degenerate=False):
    """B clouds of one shared scene array; cloud b is stretched 3x along axis b % 3, so the largest extent is on each axis in turn.
    degenerate: every id of cloud 0 is the same point (extent 0, divisor 1e-15f)."""
    rng = np.random.default_rng(1000 + seed)
    n_obj = 3000
    objs = [_object(n_obj, 200 + b) for b in range(max(B, 3))]
    xyz, nrm = [], []
    for b, o in enumerate(objs):
        c = o['xyz'].mean(axis=0)
        s = np.ones(3)
        s[b % 3] = 3.0
        xyz.append((o['xyz'] - c) * s + c)
        nrm.append(o['normal'])
    xyz64, nrm64 = np.concatenate(xyz), np.concatenate(nrm)
    ids = np.stack([b * n_obj + rng.choice(n_obj, n_pts, replace=n_obj < n_pts) for b in range(B)]).astype(np.int32)
    if degenerate:
        ids[0, :] = ids[0, 0]
    mean64, std64, mean32, inv_std32 = _normaliser(rng, with_mean)
    return {'xyz64': xyz64, 'nrm64': nrm64, 'xyz32': xyz64.astype(f32), 'nrm32': nrm64.astype(f32), 'ids': ids,
            'mean64': mean64, 'std64': std64, 'mean32': mean32, 'inv_std32': inv_std32}


# ------------------------------------------------------------------------------------------------------------ softmax_pg
def softmax_case(B, C, seed=0):
    """logits (B,C) float32 and {row: label} of the planted rows: row 0 large logits (+-80), row 1 all equal, row 2 an exact tie of
    the two largest (the label is the first), row 3 its maximum in the last class (as many of them as B holds)."""
    rng = np.random.default_rng(2000 + 37 * B + C)
    x = (rng.standard_normal((B, C)) * 3).astype(f32)
    planted = {}
    if B > 0:
        x[0] = np.where(np.arange(C) % 2 == 0, 80.0, -80.0) + rng.standard_normal(C).astype(f32)
    if B > 1:
        x[1] = f32(1.25)
        planted[1] = 0
    if B > 2 and C >= 2:
        i, j = sorted(rng.choice(C, 2, replace=False))
        x[2, i] = x[2, j] = np.abs(x[2]).max() + f32(1.5)
        planted[2] = int(i)
    if B > 3:
        x[3, C - 1] = np.abs(x[3]).max() + f32(2.0)
        planted[3] = C - 1
    return x, planted


def check_softmax(logits, planted, probs, label, conf, p_g, prob_bound, what):
    """cg_softmax_pg against transforms_ref.softmax / p_G in float64.  prob_bound: absolute bound on a probability (measured, see
    test_prep_kernels_gpu.py; the device expf is not correctly rounded).
      * probs within prob_bound;
      * label = the float64 argmax wherever the float64 top-2 probabilities differ by more than prob_bound, and the planted label
        on the planted rows (ties take the first maximum: equal logits give equal bytes);
      * conf = probs[label] bit for bit;
      * p_g = fl(chain of C fmaf(p_k, k, .)) / C: |p_g - ref| <= (prob_bound sum k + gamma_(C+1) sum (p_k + prob_bound) k) / C.
    -> worst |probs - float64| in units of u."""
    x = np.asarray(logits, f32).astype(np.float64)
    B, C = x.shape
    ref = tref.softmax(x, axis=1)
    err = np.abs(np.asarray(probs, np.float64) - ref)
    worst = float(err.max() / U32)
    assert err.max() <= prob_bound, f'{what}: probability off by {worst:.2f} u at {np.unravel_index(err.argmax(), err.shape)}, bound {prob_bound / U32:.2f} u'
    label = np.asarray(label)
    assert ((label >= 0) & (label < C)).all(), f'{what}: label out of range'
    srt = np.sort(ref, axis=1)
    clear = np.ones(B, bool) if C == 1 else (srt[:, -1] - srt[:, -2]) > prob_bound
    bad = clear & (label != ref.argmax(axis=1))
    assert not bad.any(), f'{what}: label of row {int(np.argmax(bad))} is {label[np.argmax(bad)]}, float64 argmax {ref.argmax(axis=1)[np.argmax(bad)]}'
    for row, lab in planted.items():
        assert label[row] == lab, f'{what}: planted row {row} has label {label[row]}, expected {lab}'
    R.check_bitwise(conf, np.asarray(probs, f32)[np.arange(B), label], what + ' conf vs probs[label]')
    k = np.arange(C, dtype=np.float64)
    pg_bound = (prob_bound * k.sum() + gamma(C + 1) * ((ref + prob_bound) * k).sum(axis=1)) / C + TINY
    R.check_bound(p_g, tref.p_G(ref, C), pg_bound, what + ' p_g')
    return worst


# ------------------------------------------------------------------------------------------------- sdf_points_inside_batch
def inside_neg(grid, gx, gy, gz, half_up=False, clamp_first=False):
    """inside_neg of csrc/sdf.hip on float32 grid coordinates: rint (half to even), the range test on the rounded float (no
    clamp: a point that rounds to nx is outside), grid < 0.  half_up / clamp_first: planted defects."""
    grid = np.asarray(grid, f32)
    dims = grid.shape
    with np.errstate(invalid='ignore'):
        r = [(np.floor(g + f32(0.5)) if half_up else np.rint(g)).astype(f32) for g in (gx, gy, gz)]
        if clamp_first:
            r = [np.clip(v, f32(0), f32(d - 1)) for v, d in zip(r, dims)]
        ok = np.ones(r[0].shape, bool)
        for v, d in zip(r, dims):
            ok &= (v >= f32(0)) & (v < f32(d))
    i, j, k = (np.where(ok, v, 0).astype(np.int64) for v in r)
    return ok & (grid[i, j, k] < 0)


def sdf_grid_coords(xf12, pts):
    """The three fmaf chains of sdf_points_inside_batch_kernel: xf12 (E,12), pts (P,3) float32 -> three (E,P) float32."""
    T = np.asarray(xf12, f32)[:, None, :]
    p = np.asarray(pts, f32)
    x, y, z = p[None, :, 0], p[None, :, 1], p[None, :, 2]
    return [fmaf(T[..., 4 * j], x, fmaf(T[..., 4 * j + 1], y, fmaf(T[..., 4 * j + 2], z, T[..., 4 * j + 3]))) for j in range(3)]


def sdf_inside_chain(grid, xf12, pts, chunk=1 << 18, **defect):
    """cg_sdf_points_inside_batch exactly: out[e] = any point of pts inside a negative voxel of candidate e's grid, uint8 (E,)."""
    xf12 = np.asarray(xf12, f32).reshape(-1, 12)
    pts = np.asarray(pts, f32).reshape(-1, 3)
    E, P = len(xf12), len(pts)
    out = np.zeros(E, np.uint8)
    if P == 0:
        return out
    step = max(1, chunk // P)
    for e0 in range(0, E, step):
        gx, gy, gz = sdf_grid_coords(xf12[e0:e0 + step], pts)
        out[e0:e0 + step] = inside_neg(grid, gx, gy, gz, **defect).any(axis=1)
    return out


def sdf_pose_case(E, sigma, seed, P=3000):
    """The inputs of test_sdf_gpu.py::test_batched_candidate_inside_check: scene points N(0, 0.01) about (0, 0, 0.6) rounded to
    float32, E gripper poses of random rotation and offset N(0, sigma).  -> (poses (E,4,4) float64, pts (P,3) float32)."""
    rng = np.random.default_rng(seed)
    pts = rng.normal(0, 0.01, (P, 3)) + np.array([0.0, 0.0, 0.6])
    poses = []
    for _ in range(E):
        T = np.eye(4)
        T[:3, :3] = synth.random_rotation(rng)
        T[:3, 3] = np.array([0, 0, 0.6]) + rng.normal(0, sigma, 3)
        poses.append(T)
    return np.array(poses), pts.astype(f32)


def sdf_classify(data, T_world_grid, poses, pts, chunk=64):
    """What float64 alone decides about Sdf3D.is_any_points_inside_batch.  The device evaluates the float32 rounding of
    xf = T_world_grid inv(pose) on float32 points by the fmaf chain, so its grid coordinates lie within
        delta = (gamma_4 + 2u) (|xf| |p| + |t|)   (+ 1e-9 for the float64 evaluation itself)
    of the float64 ones, per axis.  Per candidate -> 1: forced inside (some point rounds into a negative voxel and lies farther than
    delta from every rounding boundary, the grid's edges among them); 0: forced outside (no point reaches a negative voxel even
    when moved by +-delta per axis); -1: undecided.  Also -> the float64 oracle's own verdicts (sdf_ref.is_any_points_inside)."""
    data = np.asarray(data, np.float64)
    dims = np.array(data.shape)
    neg = np.zeros(tuple(dims + 2), bool)              # padded by one voxel of "outside" on every side
    neg[1:-1, 1:-1, 1:-1] = data < 0
    poses = np.asarray(poses, np.float64).reshape(-1, 4, 4)
    p = np.asarray(pts, f32).astype(np.float64)
    xf = (np.asarray(T_world_grid)[None] @ np.linalg.inv(poses))[:, :3, :]
    cls = np.empty(len(poses), np.int64)
    oracle = np.empty(len(poses), bool)

    def lookup(r):                                      # r (...,3) integer-valued floats -> negative voxel there (False outside)
        i = np.clip(r, -1, dims).astype(np.int64) + 1
        return neg[i[..., 0], i[..., 1], i[..., 2]]
    for e0 in range(0, len(poses), chunk):
        A, t = xf[e0:e0 + chunk, :, :3], xf[e0:e0 + chunk, :, 3]
        g = np.einsum('eij,pj->epi', A, p) + t[:, None, :]
        delta = (gamma(4) + 2 * U32) * (np.einsum('eij,pj->epi', np.abs(A), np.abs(p)) + np.abs(t)[:, None, :]) + 1e-9
        r = np.rint(g)
        sure = (np.abs(g - r) < 0.5 - delta).all(axis=-1)
        forced1 = (lookup(r) & sure).any(axis=1)
        lo, hi = np.rint(g - delta), np.rint(g + delta)
        reach = np.zeros(g.shape[:2], bool)
        for c in range(8):
            pick = np.stack([(hi if (c >> a) & 1 else lo)[..., a] for a in range(3)], axis=-1)
            reach |= lookup(pick)
        cls[e0:e0 + chunk] = np.where(forced1, 1, np.where(reach.any(axis=1), -1, 0))
        for k in range(len(g)):
            oracle[e0 + k] = sdf_ref.is_any_points_inside(data, g[k].T)
    return cls, oracle


def check_sdf_batch(got, cls, what, cap=0.01):
    """The rule of the batched inside check: every forced candidate agrees, and at most `cap` of the candidates are undecided."""
    got = np.asarray(got).astype(bool)
    und = cls < 0
    assert und.mean() <= cap, f'{what}: {int(und.sum())} of {len(cls)} candidates undecided in float64'
    bad = ~und & (got != (cls == 1))
    assert not bad.any(), f'{what}: candidates {np.nonzero(bad)[0][:8].tolist()} disagree with what float64 forces'
    return int(und.sum())


def sdf_planted_case():
    """Planted candidates on a small non-cubic grid (7, 5, 6), every chain exact: identity rotation, integer translation, points
    on integer, .5 and .25 coordinates far apart, so that under one candidate's translation only its own point comes near the grid.
    Column (x, 2, 3) of the grid reads  - + - + + - -  for x = 0..6.
    -> (grid float32, xf (E,12) float32, pts (70,3) float32, expected (E,) uint8, names)."""
    rng = np.random.default_rng(5)
    grid = np.abs(rng.standard_normal((7, 5, 6))).astype(f32) + f32(0.1)         # everything outside ...
    grid[:, 2, 3] = np.array([-1, 1, -1, 1, 1, -1, -1], f32)                     # ... but these
    grid[1, 0, 3] = grid[1, 4, 3] = grid[1, 1, 0] = grid[1, 1, 5] = -1
    P = 70
    pts = np.zeros((P, 3), f32)
    pts[:, 0] = 5000 + np.arange(P)                                               # filler: never near the grid
    O, H, Q, A, B = 3, 10, 20, 64, 69
    pts[O], pts[H], pts[Q] = (2000, 0, 0), (1000.5, 0, 0), (2999.75, 0, 0)
    pts[A], pts[B] = (4000, 0, 0), (-4000, 0, 0)
    cand = [  # name, point, grid coordinate it must reach, expected
        ('only-the-last-point', B, (2, 2, 3), 1),
        ('only-the-first-point-of-the-partial-round', A, (2, 2, 3), 1),
        ('half-even-down', H, (2.5, 2, 3), 1),            # rint 2 (negative); half-up 3 (positive)
        ('half-even-down-outside', H, (4.5, 2, 3), 0),    # rint 4 (positive); half-up 5 (negative)
        ('half-even-up', H, (1.5, 2, 3), 1),              # rint 2
        ('rounds-to-minus-zero', Q, (-0.25, 2, 3), 1),    # rint -0: in range, voxel 0
        ('half-rounds-to-minus-zero', H, (-0.5, 2, 3), 1),
        ('rounds-to-nx', Q, (6.75, 2, 3), 0),             # rint 7 = nx: outside, not clamped to 6 (negative)
        ('beyond-x-low', O, (-1, 2, 3), 0), ('beyond-x-high', O, (7, 2, 3), 0),
        ('beyond-y-low', O, (1, -1, 3), 0), ('beyond-y-high', O, (1, 5, 3), 0),
        ('beyond-z-low', O, (1, 1, -1), 0), ('beyond-z-high', O, (1, 1, 6), 0),
        ('edge-y-low', O, (1, 0, 3), 1), ('edge-y-high', O, (1, 4, 3), 1), ('edge-z-low', O, (1, 1, 0), 1), ('edge-z-high', O, (1, 1, 5), 1),
        ('nothing-near', O, (3, 2, 3), 0),
    ]
    xf = np.zeros((len(cand), 12), f32)
    xf[:, 0] = xf[:, 5] = xf[:, 10] = 1
    for e, (_, k, goal, _) in enumerate(cand):
        t = np.array(goal, np.float64) - pts[k].astype(np.float64)
        assert (t == np.rint(t)).all()                                            # integer grid offset
        xf[e, 3::4] = t
    return grid, xf, pts, np.array([c[3] for c in cand], np.uint8), [c[0] for c in cand]


def sdf_random_case(E, P, seed=0):
    """General candidates in grid units: a sphere of negative voxels in a (24, 17, 20) grid, points N(0, 5) voxels (N(0, 1) when P > 100), E random
    rotations scaled by U(0.5, 1.5) with translations about the centre.  xf is float32 and goes to the C function as it is.
    -> (grid, xf (E,12), pts (P,3))."""
    rng = np.random.default_rng(3000 + 7 * E + P)
    dims = np.array([24, 17, 20])
    c = (dims - 1) / 2.0
    I, J, K = np.meshgrid(*(np.arange(d) for d in dims), indexing='ij')
    grid = (np.sqrt((I - c[0]) ** 2 + (J - c[1]) ** 2 + (K - c[2]) ** 2) - 6.5).astype(f32)
    pts = rng.normal(0, 5.0 if P <= 100 else 1.0, (P, 3)).astype(f32)      # a large cloud is kept tight: else every candidate is inside
    q = rng.normal(size=(E, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    w, x, y, z = q.T
    Rm = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w),
                   2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                   2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], axis=1).reshape(E, 3, 3)
    Rm = Rm * rng.uniform(0.5, 1.5, (E, 1, 1))
    t = c + rng.normal(0, 6.0 if P <= 100 else 5.0, (E, 3))
    xf = np.concatenate([Rm, t[:, :, None]], axis=2).reshape(E, 12).astype(f32)
    return grid, xf, pts
