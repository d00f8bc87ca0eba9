"""Float64 numpy brute force for the radius queries of the grid index (include/catgrasp_amd_neighbors.h), and the clouds its tests share.

In range: d2 = (dx*dx + dy*dy) + dz*dz <= radius*radius, float64 from the given coordinates, d = p_j - q; exact ties go to the smaller
index.  The normals of an unorganized cloud are scene_ref.organized_normals as it stands: it is the windowless restatement over a
point list."""
import functools

import numpy as np

import scene_ref as R


def d2_matrix(Q, P):
    """(len(Q), len(P)) float64 d2 with the pinned expression."""
    d = P.astype(np.float64)[None, :, :] - Q.astype(np.float64)[:, None, :]
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def nearest_within(P, Q, radius, chunk=512):
    """-> index (M) int32, -1 without a point in range; d2 (M) float64, +inf there.  np.argmin takes the first minimum: the smaller index."""
    idx, d2 = np.full(len(Q), -1, np.int32), np.full(len(Q), np.inf)
    if len(P) == 0:
        return idx, d2
    for a in range(0, len(Q), chunk):
        m = d2_matrix(Q[a:a + chunk], P)
        j = np.argmin(m, axis=1)
        best = m[np.arange(len(j)), j]
        ok = best <= radius * radius
        idx[a:a + chunk] = np.where(ok, j, -1)
        d2[a:a + chunk] = np.where(ok, best, np.inf)
    return idx, d2


def count_within(P, Q, radius, chunk=512):
    """-> (M) int32 number of points of P in range of every query."""
    out = np.zeros(len(Q), np.int32)
    if len(P) == 0:
        return out
    for a in range(0, len(Q), chunk):
        out[a:a + chunk] = (d2_matrix(Q[a:a + chunk], P) <= radius * radius).sum(axis=1)
    return out


def cloudA_minus_cloudB(A, B, thres):
    """Utils.cloudA_minus_cloudB -> (A[keep], keep), keep ascending: the points of A without a point of B in range."""
    keep = np.nonzero(count_within(B, A, thres) == 0)[0]
    return A[keep], keep


@functools.lru_cache(maxsize=None)
def sheet_cloud():
    """A cloud that never was an image: 6,000 points on a noisy wavy sheet, 1,500 on a noisy sphere, two lone points far outside;
    float32, shuffled.  Shared: never written to."""
    rng = np.random.default_rng(5)
    uv = rng.uniform(-0.03, 0.03, (6000, 2))
    z = 0.6 + 0.004 * np.sin(90 * uv[:, 0]) * np.cos(70 * uv[:, 1]) + rng.normal(0, 3e-5, 6000)
    sheet = np.column_stack((uv, z))
    d = rng.normal(size=(1500, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    sphere = np.array([0.05, -0.02, 0.55]) + d * (0.008 + rng.normal(0, 2e-5, (1500, 1)))
    lone = np.array([[0.2, 0.2, 0.9], [-0.3, 0.1, 0.4]])
    P = np.concatenate((sheet, sphere, lone)).astype(np.float32)
    P = P[rng.permutation(len(P))]
    P.setflags(write=False)
    return P


def mm_lattice(dtype):
    """13^3 points at (i, j - 3, k + 500) * 0.001, i, j, k in -6..6: at radius 0.002 the pairs two steps apart fall on either side of the
    bound, by rounding alone."""
    g = np.arange(-6, 7)
    i, j, k = np.meshgrid(g, g - 3, g + 500, indexing='ij')
    return (np.stack((i, j, k), -1).reshape(-1, 3) * 0.001).astype(dtype)


def pow2_lattice():
    """9^3 points at spacing 2^-10 shifted by (0, -2, 512) steps: every coordinate and every d2 is exact, so d2 == r^2 happens (r = 2^-9)."""
    g = np.arange(9)
    i, j, k = np.meshgrid(g, g - 2, g + 512, indexing='ij')
    return np.stack((i, j, k), -1).reshape(-1, 3) * 2.0 ** -10


@functools.lru_cache(maxsize=None)
def cloud(name):
    """The named test clouds, shared and read-only.  'A', 'B': the used points of scene_ref's scenes in row-major order; 'A_perm',
    'B_perm': the same points shuffled; 'sheet': sheet_cloud()."""
    if name == 'sheet':
        return sheet_cloud()
    if name.endswith('_perm'):
        P = cloud(name[0])
        P = P[np.random.default_rng({'A': 11, 'B': 12}[name[0]]).permutation(len(P))]
    else:
        depth, bg, K = (*R.scene_a(), R.K_A) if name == 'A' else (R.scene_b(), None, R.K_B)
        xyz, valid = R.depth2xyzmap(depth, K)
        P = xyz[valid if bg is None else valid & ~bg]
    P.setflags(write=False)
    return P


@functools.lru_cache(maxsize=None)
def pairs(name, radius):
    return R.in_range_pairs(cloud(name), radius)


@functools.lru_cache(maxsize=None)
def normals_ref(name, radius=0.002, max_nn=30, prefer='low'):
    """scene_ref.organized_normals of the named cloud as a point list."""
    return R.organized_normals(cloud(name), radius, max_nn, prefer=prefer, pairs=pairs(name, radius))
