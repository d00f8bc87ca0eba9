"""Float64 numpy restatement of the scene front end (include/catgrasp_amd_scene.h) and the scenes its tests share.

depth2xyzmap restates Utils.depth2xyzmap (pinned bit for bit against the reference function by tests/golden/scene_golden.npz).
organized_normals restates the pinned semantics of cg_organized_normals WITHOUT the pixel window: brute-force neighbours over all
used points, in chunks; np.linalg.eigh on a two-pass covariance.  It is not pinned against open3d."""
import numpy as np

K_A = np.array([[2257.75, 0, 40.3], [0, 2257.49, 30.7], [0, 0, 1]])
K_B = np.array([[2048.0, 0, 20], [0, 2048.0, 20], [0, 0, 1]])


def depth2xyzmap(depth, K):
    """-> xyz_map (H, W, 3) float32, valid (H, W) bool."""
    invalid = depth < 0.1                                   # in the depth's own dtype
    H, W = depth.shape
    vs, us = np.meshgrid(np.arange(0, H), np.arange(0, W), sparse=False, indexing='ij')
    zs = depth.astype(np.float64)
    xs = (us - K[0, 2]) * zs / K[0, 0]
    ys = (vs - K[1, 2]) * zs / K[1, 1]
    xyz = np.stack((xs, ys, zs), -1).astype(np.float32)
    xyz[invalid] = 0
    return xyz, ~invalid


def scene_a(seed=3, near_patch=False):
    """72 x 96 pixels: a tilted plane with a dent, a step, a far noise-free patch, holes, a lone pixel, and a background mask.
    -> depth (float32), bg_mask (bool).  near_patch adds a 10 x 10 patch at z = 0.12, whose window half-width is about 40 pixels."""
    H, W = 72, 96
    rng = np.random.default_rng(seed)
    v, u = np.meshgrid(np.arange(H), np.arange(W), indexing='ij')
    z = 0.55 + 0.0006 * (u - 48) + 0.0004 * (v - 36)
    rho2 = (u - 30.0) ** 2 + (v - 30.0) ** 2
    z = z + 0.003 * np.sqrt(np.clip(1 - rho2 / 18.0 ** 2, 0, None))     # a spherical dent of radius 18 px at (30, 30)
    z[:, 70:] += 0.25                                       # a step to z ~ 0.80
    if near_patch:
        z[30:40, 50:60] = 0.12
    z = z + rng.normal(0, 2e-5, z.shape)
    z[50:, :30] = 2.9                                       # noise-free; the pixel pitch there is 1.3 mm
    z[10:14, 50:62] = 0.0                                   # a hole
    z[20, 60] = 0.05                                        # below the validity threshold
    z[5, 80] = 0.30                                         # a lone pixel: nothing else within the radius
    bg = np.zeros((H, W), bool)
    bg[:, 92:] = True
    bg[40:44, 40:46] = True
    return z.astype(np.float32), bg


def scene_b():
    """40 x 40 pixels whose coordinates are exact in float32, so that ties at the 30th place are exact.  -> depth (float32)."""
    u = np.arange(40)
    z = np.where(u % 3 == 0, 0.5 + 2.0 ** -12, 0.5)
    return np.broadcast_to(z, (40, 40)).astype(np.float32).copy()


def in_range_pairs(P, radius, chunk=512):
    """All (q, j, d2) with d2 = (dx*dx + dy*dy) + dz*dz <= radius*radius, float64 from the given coordinates, q-major, j ascending."""
    P = P.astype(np.float64)
    r2 = radius * radius
    qs, js, ds = [], [], []
    for a in range(0, len(P), chunk):
        d = P[None, :, :] - P[a:a + chunk, None, :]
        d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        q, j = np.nonzero(d2 <= r2)
        qs.append(q + a); js.append(j); ds.append(d2[q, j])
    return np.concatenate(qs), np.concatenate(js), np.concatenate(ds)


def organized_normals(P, radius=0.002, max_nn=30, view_point=(0.0, 0.0, 0.0), prefer='low', pairs=None):
    """P: (N, 3) float32 used points in row-major pixel order.  -> dict(count (N) int, d2max (N), normals (N,3), raw (N,3), C (N,3,3),
    lam (N,3) ascending eigenvalues (zeros where count < 3), tie (N) bool: an exact tie between the last neighbour taken and the first
    one left out, gap (N): relative gap between those two d2 (inf where nothing is left out), pairs).  prefer: 'low' gives exact ties
    at the last place to the smaller index (the pinned rule), 'high' to the larger."""
    N = len(P)
    P64 = P.astype(np.float64)
    q, j, d2 = in_range_pairs(P, radius) if pairs is None else pairs
    order = np.lexsort((j if prefer == 'low' else -j, d2, q))
    q, j, d2 = q[order], j[order], d2[order]
    start = np.searchsorted(q, np.arange(N))
    total = np.diff(np.append(start, len(q)))
    rank = np.arange(len(q)) - start[q]
    count = np.minimum(total, max_nn)
    kmax = int(count.max())
    take = rank < max_nn
    idx = np.full((N, kmax), -1)
    idx[q[take], rank[take]] = j[take]
    dd = np.zeros((N, kmax))
    dd[q[take], rank[take]] = d2[take]
    d2max = dd.max(axis=1)
    nxt = np.full(N, np.inf)                                # d2 of the first candidate left out
    first_out = rank == max_nn
    nxt[q[first_out]] = d2[first_out]
    tie = nxt == d2max
    with np.errstate(invalid='ignore', divide='ignore'):
        gap = np.where(np.isfinite(nxt), (nxt - d2max) / nxt, np.inf)
    m = idx >= 0
    pts = np.where(m[..., None], P64[np.where(m, idx, 0)], 0.0)
    n = count.astype(np.float64)[:, None]
    mean = pts.sum(axis=1) / n
    dev = np.where(m[..., None], pts - mean[:, None, :], 0.0)
    C = np.einsum('nki,nkj->nij', dev, dev) / n[:, :, None]
    lam, vec = np.linalg.eigh(C)
    raw = vec[:, :, 0].copy()
    few = count < 3
    raw[few] = (0.0, 0.0, 1.0)
    lam = np.where(few[:, None], 0.0, lam)
    # correct_pcd_normal_direction
    view = np.asarray(view_point, dtype=np.float64).reshape(-1, 3) - P64
    view = view / np.linalg.norm(view, axis=1).reshape(-1, 1)
    normals = raw / (np.linalg.norm(raw, axis=1) + 1e-10).reshape(-1, 1)
    flip = (view * normals).sum(axis=1) < 0
    normals[flip] = -normals[flip]
    return dict(count=count.astype(np.int32), d2max=d2max, normals=normals, raw=raw, C=C, lam=lam, tie=tie & (total > max_nn), gap=gap,
                view=view, pairs=(q, j, d2))


def window_halfwidths(xyz_map, K, radius):
    """Per pixel, the window bound of the header: ceil((fx + |u - cx|) * radius / (z - radius)) + 1 in u, likewise in v (the whole
    image where z <= radius).  -> hu, hv (H, W) float64."""
    H, W = xyz_map.shape[:2]
    z = xyz_map[..., 2].astype(np.float64) - radius
    v, u = np.meshgrid(np.arange(H), np.arange(W), indexing='ij')
    with np.errstate(invalid='ignore', divide='ignore'):
        hu = np.where(z > 0, np.ceil((K[0, 0] + np.abs(u - K[0, 2])) * radius / z) + 1, max(H, W))
        hv = np.where(z > 0, np.ceil((K[1, 1] + np.abs(v - K[1, 2])) * radius / z) + 1, max(H, W))
    return hu, hv
