"""Constructed inputs for the pairwise collision kernels of csrc/collision_pairs.hip (numpy only: no GPU, no oracle).

Every case carries its verdict from the construction and, where a single pair decides it, a minus variant: the same case with the
deciding shape moved one lattice step out of contact (or far away, where it overlaps instead of touching); the minus verdict is False.

Exactness.  Mesh coordinates are integers in units of RES = 2**-11 with |coordinate| < 2048 (so |x| < 1); poses are proper
signed-permutation rotations with lattice translations, neither of them the identity.  The fma pose chain then returns lattice
points, and with a pair's vertices within 16 units of one another every edge (<= 2**5), normal (<= 2**11), in-plane axis (<= 2**17)
and projection (< 2**24) of the kernel's separating-axis test is an integer of fewer than 24 bits times a power of two: float32
computes it without rounding.  tests/test_pair_scenes_cpu.py proves this by running `tri_axes` in float32 and in int64.
Clouds use res_a = 2**-11 and res_b in {2**-11, 2**-10}; with an aligned `rel` the 15 box expressions are exact in the same way.  The
rotated `rel` cases are not exact; their margins are stated at ROT_MARGIN below.

Pairs of two zero-area faces are left out: the oracle returns 0 for them by fiat (segment against segment is pinned nowhere).

Numbering, as in the kernels.  Triangles: axis 0 = np, 1 = nq, 2 + 3 i + j = ep[i] x eq[j], 11 + 2 i = np x ep[i], 12 + 2 i = nq x eq[i],
and for zero-area faces 17 + i = nq x ep[i] (np == 0), 20 + i = np x eq[i] (nq == 0).  Boxes: 0..2 = A's face axes, 3..5 = B's,
6 + 3 i + j = a_i x b_j."""
import itertools

import numpy as np

RES = 2.0 ** -11
CHUNK = 256            # PB_CHUNK
CAP = 4096             # most workgroups of a launch
FAR_STEP = 24          # lattice units by which an overlapping (not touching) witness is taken away in its minus variant


def exact32(x):
    x = np.asarray(x, dtype=np.float64)
    y = x.astype(np.float32)
    assert np.array_equal(y.astype(np.float64)[~np.isnan(x)], x[~np.isnan(x)]), 'a value does not round-trip through float32'
    return y


# ---------------------------------------------------------------------------------------------------------------------------------
# poses
def sp_pose(perm, signs, t_units):
    """proper signed permutation: row r of the rotation has `signs[r]` in column perm[r]; translation in lattice units"""
    T = np.eye(4)
    T[:3, :3] = 0.0
    for r in range(3):
        T[r, perm[r]] = signs[r]
    assert abs(np.linalg.det(T[:3, :3]) - 1.0) < 1e-12 and not np.array_equal(T[:3, :3], np.eye(3))
    T[:3, 3] = np.asarray(t_units, dtype=np.float64) * RES
    return T


POSE_A = sp_pose((1, 2, 0), (1, 1, 1), (5, -3, 2))          # x <- y, y <- z, z <- x
POSE_B = sp_pose((1, 0, 2), (-1, 1, 1), (-4, 6, 1))         # a quarter turn about z


def unpose(T, W):
    """world points (units) -> mesh-frame coordinates (float64, on the lattice) under the signed-permutation pose T"""
    W = np.asarray(W, dtype=np.float64) * RES
    return (W - T[:3, 3]) @ T[:3, :3]          # R^T (w - t), row vectors


def posed(T, V):
    """the kernel's fma pose chain in float32 (exact for the lattice poses)"""
    T = np.asarray(T, dtype=np.float32); V = np.asarray(V, dtype=np.float32)
    out = np.empty_like(V)
    for r in range(3):
        out[..., r] = T[r, 0] * V[..., 0] + (T[r, 1] * V[..., 1] + (T[r, 2] * V[..., 2] + T[r, 3]))
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# the kernels' separating-axis expressions, restated (vectorised; any dtype: float32 as the kernel, int64 / float64 for the proof)
def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def tri_axes(P, Q, dtype=np.float32, swap=None, closed=None, zero_area_axes=True):
    """tri_tri_overlap of the kernel on P, Q (n,3,3).  -> (sep (n,23) bool, gap (n,23)): sep[k] = axis k separates; gap = the distance
    between the two projected intervals (negative: they overlap) in the units of the axis.  Columns 17..22 are the axes the kernel adds
    for zero-area faces.  Faulty variants for the sensitivity check: swap=(i, j) builds axis (i, j) from eq[(j + 1) % 3]; closed=k
    separates on axis k already when the intervals touch."""
    P = np.asarray(P).astype(dtype).reshape(-1, 3, 3); Q = np.asarray(Q).astype(dtype).reshape(-1, 3, 3)
    p = P - P[:, :1]; q = Q - P[:, :1]
    ep = np.roll(p, -1, axis=1) - p; eq = np.roll(q, -1, axis=1) - q
    npn = _cross(ep[:, 0], ep[:, 1]); nq = _cross(eq[:, 0], eq[:, 1])
    L = [npn, nq]
    for i in range(3):
        for j in range(3):
            L.append(_cross(ep[:, i], eq[:, (j + 1) % 3 if swap == (i, j) else j]))
    for i in range(3):
        L += [_cross(npn, ep[:, i]), _cross(nq, eq[:, i])]
    L += [_cross(nq, ep[:, i]) for i in range(3)] + [_cross(npn, eq[:, i]) for i in range(3)]
    L = np.stack(L, axis=1)                                    # (n,23,3)
    a = _dot(L[:, :, None, :], p[:, None, :, :]); b = _dot(L[:, :, None, :], q[:, None, :, :])
    amin, amax, bmin, bmax = a.min(-1), a.max(-1), b.min(-1), b.max(-1)
    sep = (amax < bmin) | (bmax < amin)
    if closed is not None:
        sep[:, closed] |= (amax[:, closed] <= bmin[:, closed]) | (bmax[:, closed] <= amin[:, closed])
    pz = np.all(npn == 0, axis=-1); qz = np.all(nq == 0, axis=-1)
    on = np.ones(sep.shape, dtype=bool)
    on[:, 17:20] = pz[:, None] & zero_area_axes; on[:, 20:23] = qz[:, None] & zero_area_axes
    return sep & on, np.maximum(bmin - amax, amin - bmax)


def tri_hit(P, Q, **kw):
    return ~tri_axes(P, Q, **kw)[0].any(axis=1)


def box_axes(t, ha, hb, R, dtype=np.float32):
    """box_box_overlap of the kernel: t (n,3) = cb - ca, R (3,3) row-major.  -> (n,15): |t.L| - (ra + rb); positive = separated."""
    t = np.asarray(t).astype(dtype).reshape(-1, 3); R = np.asarray(R).astype(dtype).reshape(3, 3)
    ha = dtype(ha); hb = dtype(hb)
    Qa = np.abs(R)
    out = []
    for i in range(3):
        out.append(np.abs(t[:, i]) - (ha + hb * ((Qa[i, 0] + Qa[i, 1]) + Qa[i, 2])))
    for j in range(3):
        tj = (t[:, 0] * R[0, j] + t[:, 1] * R[1, j]) + t[:, 2] * R[2, j]
        out.append(np.abs(tj) - (ha * ((Qa[0, j] + Qa[1, j]) + Qa[2, j]) + hb))
    for i in range(3):
        i1, i2 = (i + 1) % 3, (i + 2) % 3
        for j in range(3):
            j1, j2 = (j + 1) % 3, (j + 2) % 3
            tl = t[:, i2] * R[i1, j] - t[:, i1] * R[i2, j]
            ra = ha * Qa[i2, j] + ha * Qa[i1, j]
            rb = hb * Qa[i, j2] + hb * Qa[i, j1]
            out.append(np.abs(tl) - (ra + rb))
    return np.stack(out, axis=1)


def reach_of(res_a, res_b):
    f = np.float32
    return f(f(f(1.7320508) * f(f(0.5) * f(res_a) + f(0.5) * f(res_b))) * f(1.0001))


def centres(keys, res, dtype=np.float64):
    return ((np.asarray(keys).astype(dtype) + dtype(0.5)) * dtype(res)).reshape(-1, 3)


def cloud_t(keys_a, res_a, keys_b, res_b, rel, dtype=np.float64):
    """t = posed centre of every key of B minus the centre of every key of A -> (na, nb, 3)"""
    ca = centres(keys_a, res_a, dtype); cb = centres(keys_b, res_b, dtype)
    rel = np.asarray(rel).astype(dtype)
    o = np.stack([rel[r, 0] * cb[:, 0] + (rel[r, 1] * cb[:, 1] + (rel[r, 2] * cb[:, 2] + rel[r, 3])) for r in range(3)], axis=1)
    return o[None, :, :] - ca[:, None, :]


# ---------------------------------------------------------------------------------------------------------------------------------
# the launcher's arithmetic, restated
def launch(na, nb):
    """-> (gx, gy, per, chunks) of cg_mesh_mesh_collide / cg_voxels_voxels_collide for na x nb shapes"""
    chunks = (nb + CHUNK - 1) // CHUNK
    gx = (na + 255) // 256
    gy = chunks
    if gx * gy > CAP:
        gy = (CAP + gx - 1) // gx
    gy = max(gy, 1)
    per = (chunks + gy - 1) // gy
    gy = (chunks + per - 1) // per
    return gx, gy, per, chunks


def where(na, nb, ia, ib):
    """the workgroup, thread and chunk that meet the pair (ia, ib)"""
    gx, gy, per, chunks = launch(na, nb)
    c = ib // CHUNK
    return dict(gx=gx, gy=gy, per=per, chunks=chunks, x=ia // 256, thread=ia % 256, chunk=c, y=c // per, slot=c % per, lane=ib % CHUNK,
                last_chunk=c == chunks - 1, chunks_of_last_y=chunks - (gy - 1) * per)


# ---------------------------------------------------------------------------------------------------------------------------------
# triangle pairs, in world lattice units
class TriPair:
    """A (3,3) against B (3,3), integer world coordinates in units of RES.  `minus` is the pair out of contact (verdict False)."""

    def __init__(self, name, cls, A, B, verdict, minus=None, sole=False):
        self.name, self.cls, self.verdict, self.minus, self.sole = name, cls, bool(verdict), minus, sole
        self.A = np.asarray(A, dtype=np.int64).reshape(3, 3); self.B = np.asarray(B, dtype=np.int64).reshape(3, 3)
        za, zb = (not np.any(np.cross(t[1] - t[0], t[2] - t[0])) for t in (self.A, self.B))
        assert not (za and zb), 'pairs of two zero-area faces are left out'

    def swapped(self):
        return TriPair(self.name + '_ba', self.cls, self.B, self.A, self.verdict, self.minus.swapped() if self.minus else None, self.sole)

    def rolled(self, r, s):
        m = self.minus.rolled(r, s) if self.minus else None
        return TriPair(f'{self.name}_r{r}{s}', self.cls, np.roll(self.A, -r, axis=0), np.roll(self.B, -s, axis=0), self.verdict, m, self.sole)

    def with_minus(self):
        return [self] + ([self.minus] if self.minus is not None else [])


def sole_axis(pair):
    """the one axis (kernel numbering) that separates the pair, from the int64 restatement; asserts that it is the only one"""
    sep, _ = tri_axes(pair.A[None], pair.B[None], dtype=np.int64)
    k = np.nonzero(sep[0])[0]
    assert len(k) == 1, (pair.name, k)
    return int(k[0])


T8 = [(0, 0, 0), (8, 0, 0), (0, 8, 0)]
T_APEX = [(0, 0, 0), (-1, -2, 0), (1, -2, 0)]


def _touch(name, cls, A, B, d, verdict=True):
    """B touches (or overlaps) A; the minus variant is B moved by d (one lattice step) or, d = None, taken FAR_STEP away along z"""
    B = np.asarray(B, dtype=np.int64)
    step = np.asarray(d if d is not None else (0, 0, FAR_STEP), dtype=np.int64)
    assert d is None or np.abs(step).sum() == 1
    minus = TriPair(name + ('_apart' if d is not None else '_away'), cls, A, B + step, False)
    return TriPair(name, cls, A, B, verdict, minus)


# for every axis k of the 17: (A, B, d): A and B touch with gap 0 on axis k; with B moved by d axis k ALONE separates them
# (found by a seeded random search over integer triangles in [-5, 5]^3; coplanar ones for the in-plane axes 11..16)
TRI_SOLE = {
    0: ([[-4, -4, 3], [-5, 1, -4], [-1, -5, -4]], [[2, 1, -3], [4, -1, 0], [-4, -3, 1]], [1, 0, 0]),
    1: ([[1, 0, 0], [-4, 0, 3], [-5, 2, -3]], [[-1, 0, -1], [-1, 2, -3], [5, -2, 4]], [1, 0, 0]),
    2: ([[5, 2, 0], [-5, 1, 2], [0, -2, -5]], [[0, -1, 0], [0, 4, 2], [1, 3, 3]], [1, 0, 0]),
    3: ([[-2, 2, 0], [4, -2, 2], [-3, 5, -4]], [[-2, 3, 4], [1, 0, 1], [-3, 0, 2]], [1, 0, 0]),
    4: ([[-2, -3, -5], [2, -4, 5], [-4, -3, 2]], [[0, -4, -1], [2, 3, -2], [-1, -1, 2]], [1, 0, 0]),
    5: ([[-5, -2, 3], [5, -5, 5], [-1, 3, 0]], [[-1, -3, 4], [5, 4, -1], [2, 4, 1]], [1, 0, 0]),
    6: ([[-5, -3, 3], [-1, -2, 4], [-3, 0, -2]], [[2, -2, -3], [-4, 1, 3], [1, -4, 0]], [1, 0, 0]),
    7: ([[1, 0, 5], [4, 4, 5], [-3, -5, -3]], [[1, 5, 1], [-1, 2, -5], [2, -1, 3]], [1, 0, 0]),
    8: ([[-2, -2, 4], [-1, 4, 3], [5, 4, -1]], [[-2, -1, 3], [5, -1, 4], [1, -2, 0]], [1, 0, 0]),
    9: ([[2, -4, 2], [-5, -5, 3], [2, -1, -4]], [[-1, 5, 1], [2, -3, 0], [0, -1, -1]], [1, 0, 0]),
    10: ([[-3, -2, -3], [3, 0, 3], [4, 3, 0]], [[-4, 5, 0], [1, 3, -5], [5, -4, -3]], [1, 0, 0]),
    11: ([[-5, -2, 0], [3, -1, 0], [1, 1, 0]], [[2, -3, 0], [4, -5, 0], [-5, -2, 0]], [1, 0, 0]),
    12: ([[0, 1, 0], [-2, 5, 0], [-3, 5, 0]], [[0, -4, 0], [0, 4, 0], [4, -3, 0]], [1, 0, 0]),
    13: ([[-4, 0, 0], [-1, -3, 0], [1, 5, 0]], [[0, 1, 0], [4, 3, 0], [5, 3, 0]], [1, 0, 0]),
    14: ([[-3, 3, 0], [0, -1, 0], [1, -1, 0]], [[5, -3, 0], [3, 0, 0], [-3, -3, 0]], [1, 0, 0]),
    15: ([[1, 2, 0], [-3, 5, 0], [-3, -1, 0]], [[-2, -2, 0], [4, -5, 0], [-3, -1, 0]], [1, 0, 0]),
    16: ([[1, 0, 0], [-4, -2, 0], [2, -4, 0]], [[-3, 4, 0], [3, 1, 0], [2, -1, 0]], [1, 0, 0]),
}


def tri_contacts():
    """the contact classes, each in both argument orders"""
    out = [
        _touch('pierce', 'pierce', T8, [(2, 2, -3), (2, 2, 3), (5, 4, 3)], None),
        _touch('vertex_on_face', 'vertex-face', T8, [(2, 2, 0), (3, 2, 4), (2, 3, 4)], (0, 0, 1)),
        _touch('vertex_on_edge', 'vertex-edge', T8, [(4, 0, 0), (4, -3, 2), (5, -3, 3)], (0, -1, 0)),
        _touch('vertex_on_vertex', 'vertex-vertex', T8, [(8, 0, 0), (10, 1, 2), (10, -1, 3)], (1, 0, 0)),
        _touch('edges_cross', 'edge-edge', T8, [(4, -2, -2), (4, 2, 2), (4, -2, 2)], (0, -1, 0)),
        _touch('collinear_overlap', 'collinear', T8, [(2, 0, 0), (12, 0, 0), (6, -4, 3)], (0, -1, 0)),
        _touch('collinear_meet', 'collinear', T8, [(8, 0, 0), (14, 0, 0), (11, -4, 3)], (1, 0, 0)),       # its minus: collinear, apart
        _touch('coplanar_overlap', 'coplanar', T8, [(2, 2, 0), (12, 3, 0), (3, 12, 0)], None),
        _touch('coplanar_inside', 'coplanar', T8, [(1, 1, 0), (3, 1, 0), (1, 3, 0)], (0, 0, 1)),          # its minus: parallel planes
        _touch('coplanar_contains', 'coplanar', T8, [(-2, -2, 0), (14, -2, 0), (-2, 14, 0)], (0, 0, -1)),
        _touch('coplanar_edge', 'coplanar', T8, [(0, 0, 0), (8, 0, 0), (3, -5, 0)], (0, -1, 0)),
        _touch('coplanar_vertex', 'coplanar', T8, [(8, 0, 0), (12, -2, 0), (12, 3, 0)], (1, 0, 0)),
    ]
    return out + [p.swapped() for p in out]


def tri_zero_area():
    """a zero-area face (collinear, or all three vertices equal) against a proper triangle, both argument orders"""
    pt = lambda x, y, z: [(x, y, z)] * 3
    out = [
        _touch('segment_crosses', 'zero-area', T8, [(2, 2, -4), (2, 2, 4), (2, 2, 0)], None),
        _touch('segment_end_on_face', 'zero-area', T8, [(2, 2, 0), (2, 2, 4), (2, 2, 2)], (0, 0, 1)),
        TriPair('segment_misses_off_plane', 'zero-area', T8, [(7, 7, -4), (7, 7, 4), (7, 7, 0)], False),
        _touch('segment_in_plane_through', 'zero-area', T8, [(-2, 3, 0), (10, 3, 0), (4, 3, 0)], None),
        _touch('segment_on_edge', 'zero-area', T8, [(2, 0, 0), (6, 0, 0), (4, 0, 0)], (0, -1, 0)),        # minus: the triangle's edge normal
        # minus: the coplanar miss that only the SEGMENT's in-plane normal separates (axes 17..22)
        _touch('segment_past_apex', 'zero-area-own-normal', T_APEX, [(-8, -2, 0), (8, 2, 0), (0, 0, 0)], (0, 1, 0)),
        _touch('segment_past_apex_mid_first', 'zero-area-own-normal', T_APEX, [(0, 0, 0), (-8, -2, 0), (8, 2, 0)], (0, 1, 0)),
        _touch('point_on_face', 'zero-area', T8, pt(2, 2, 0), (0, 0, 1)),
        _touch('point_on_edge_in_plane', 'zero-area', T8, pt(4, 4, 0), (1, 0, 0)),
        _touch('point_on_vertex', 'zero-area', T8, pt(8, 0, 0), (1, 0, 0)),
    ]
    return out + [p.swapped() for p in out]


def tri_sole():
    """for each of the 17 axes: the touching twin (True) whose minus only this axis separates -- in both argument orders and under every
    vertex rotation of both faces (the deciding axis of each variant: `sole_axis(pair.minus)`)"""
    out = []
    for k, (A, B, d) in TRI_SOLE.items():
        base = _touch(f'sole{k}', 'sole', A, B, d)
        base.sole = base.minus.sole = True
        for p in (base, base.swapped()):
            out += [p.rolled(r, s) for r in range(3) for s in range(3)]
    return out


def tri_catalogue():
    return tri_contacts() + tri_zero_area() + tri_sole()


# ---------------------------------------------------------------------------------------------------------------------------------
# mesh scenes
class MeshScene:
    def __init__(self, name, cls, VA, FA, VB, FB, verdict, wit=None, minus=None, pair=None, pose_a=POSE_A, pose_b=POSE_B):
        self.name, self.cls, self.verdict, self.wit, self.minus, self.pair = name, cls, bool(verdict), wit, minus, pair
        self.VA, self.VB = exact32(VA), exact32(VB)
        self.FA, self.FB = np.ascontiguousarray(FA, dtype=np.int32), np.ascontiguousarray(FB, dtype=np.int32)
        self.pose_a, self.pose_b = exact32(pose_a), exact32(pose_b)
        for V in (self.VA, self.VB):
            assert np.nanmax(np.abs(V), initial=0.0) < 1.0
        self.capped = launch(len(self.FA), len(self.FB))[2] >= 2

    @property
    def shape(self):
        return len(self.FA), len(self.FB)

    def world(self, side):
        """posed triangles (n,3,3) float32, as the kernel poses them"""
        V, F, T = (self.VA, self.FA, self.pose_a) if side == 0 else (self.VB, self.FB, self.pose_b)
        return posed(T, V[F])

    def with_minus(self):
        return [self] + ([self.minus] if self.minus is not None else [])


W_WITNESS = np.array([-40, -40, -40])                       # where the witness pair sits; the fillers fill x, y, z >= -1
FILL_A = np.array([(0, 0, 0), (4, 0, 0), (0, 4, 0)])
FILL_B = np.array([(3, 3, -1), (4, 3, 1), (3, 4, 1)])       # inside FILL_A's box, beyond its hypotenuse: boxes overlap, shapes do not
CAPPED_SHIFT = np.array([400, 0, 0])                        # the capped shape's B fillers: all box-rejected


def _cells(n, wide):
    c = np.arange(n)
    return np.stack([c % wide, (c // wide) % wide, c // (wide * wide)], axis=1) * 8


def _indexed(tris, wi):
    """(n,3,3) -> V, F: a shared vertex array in sorted (not face) order, every sixth row unreferenced (NaN), the witness face's three
    vertices last behind another NaN row"""
    n = len(tris)
    others = np.delete(np.arange(n), wi) if wi is not None else np.arange(n)
    uniq, inv = np.unique(tris[others].reshape(-1, 3), axis=0, return_inverse=True)
    pos = np.arange(len(uniq)); pos = pos + pos // 5 + 1
    nfill = int(pos[-1]) + 1 if len(uniq) else 0
    V = np.full((nfill + (4 if wi is not None else 1), 3), np.nan)
    V[pos] = uniq
    F = np.zeros((n, 3), dtype=np.int32)
    F[others] = pos[np.asarray(inv).reshape(-1)].reshape(-1, 3)
    if wi is not None:
        V[-3:] = tris[wi]
        F[wi] = [len(V) - 3, len(V) - 2, len(V) - 1]
    return V, F


def mesh_scene(pair, na=1, nb=1, ia=0, ib=0, cls=None, name=None):
    """`pair` as face ia of A and face ib of B among na - 1 and nb - 1 fillers.  Filler c of A and filler c of B share a cell: their
    boxes overlap, the shapes do not.  In a capped shape (per >= 2) B's fillers are moved off: every filler pair is box-rejected."""
    capped = launch(na, nb)[2] >= 2
    wide = 40 if capped else 16
    ta = _cells(na - 1, wide)[:, None, :] + FILL_A[None]
    tb = _cells(nb - 1, wide)[:, None, :] + FILL_B[None] + (CAPPED_SHIFT if capped else 0)
    ta = np.insert(ta, ia, pair.A + W_WITNESS, axis=0); tb = np.insert(tb, ib, pair.B + W_WITNESS, axis=0)
    VA, FA = _indexed(ta, ia); VB, FB = _indexed(tb, ib)
    name = name or f'{pair.name}_{na}x{nb}_at{ia}_{ib}'
    minus = mesh_scene(pair.minus, na, nb, ia, ib, cls, name + '_minus') if pair.minus is not None else None
    s = MeshScene(name, cls or pair.cls, unpose(POSE_A, VA), FA, unpose(POSE_B, VB), FB, pair.verdict, (ia, ib) if pair.verdict else None,
                  minus, pair)
    s.at = (ia, ib)                                            # where the pair sits, in the minus variant too
    return s


def mesh_self_scene(n=1025):
    """all pairs hit: a mesh against itself in the same pose (every face meets itself)"""
    V, F = _indexed(_cells(n, 16)[:, None, :] + FILL_A[None], None)
    return MeshScene(f'mesh_self_{n}', 'all-pairs', unpose(POSE_A, V), F, unpose(POSE_A, V), F, True, pose_b=POSE_A)


# ---- the positions the traversal scenes reach
NA_LIST = (1, 255, 256, 257, 513)
NB_LIST = (257, 511, 512, 513, 767, 768)                   # 2 and 3 chunks; nb % 256 in {1, 255, 0}
CAPPED_NA, CAPPED_NB = 4097, 61953                          # gx = 17, chunks = 243 > 4096 / 17: per = 2, gy = 122, the last workgroup has 1 chunk


def traversal_positions():
    a = [(na, ia) for na in NA_LIST for ia in sorted({i for i in (0, 63, 64, 255, 256, na - 1) if i < na})]
    b = [(nb, ib) for nb in NB_LIST for ib in (0, 255, 256, nb - 1)]
    return [a[i % len(a)] + b[i] for i in range(len(b))]


def capped_positions():
    """witness of B in the first chunk of a workgroup, in the second, in the last chunk overall; witness of A in the first and in the
    last grid.x workgroup"""
    ibs = (100 * CHUNK + 17, 101 * CHUNK + 200, CAPPED_NB - 1)
    return [(CAPPED_NA, ia, CAPPED_NB, ib) for ia in (5, CAPPED_NA - 1) for ib in ibs]


TRAVERSAL_PAIR = 'vertex_on_face'


def _contact(name):
    return {p.name: p for p in tri_contacts()}[name]


_memo = {}


def _once(key, fn):
    if key not in _memo:
        _memo[key] = fn()
    return _memo[key]


def mesh_traversal_scenes():
    return _once('mt', lambda: [mesh_scene(_contact(TRAVERSAL_PAIR), na, nb, ia, ib, cls='traversal') for na, ia, nb, ib in traversal_positions()])


def mesh_capped_scenes():
    return _once('mc', lambda: [mesh_scene(_contact(TRAVERSAL_PAIR), na, nb, ia, ib, cls='capped') for na, ia, nb, ib in capped_positions()])


EMBED = (257, 513, 193, 300)                                # na, nb, ia, ib: thread 193 of workgroup 0, chunk 1, lane 44


def mesh_catalogue_scenes(embedded=False):
    if embedded:
        return _once('me', lambda: [mesh_scene(p, *EMBED) for p in tri_catalogue()])
    return _once('m1', lambda: [mesh_scene(p) for p in tri_catalogue()])


# ---------------------------------------------------------------------------------------------------------------------------------
# cube pairs
RES_A = RES
ROT_MARGIN = 2.0 ** -10      # every one of the 15 expressions of a rotated pair, in float64 on the float32 inputs, is at least
#                              ROT_MARGIN * (ha + hb) from zero.
# The kernel's float32 rounding of those expressions, with u = 2**-24, h = ha + hb, every value of the pose chain within 16 h (asserted
# by the builder: |translation| + sum |R| |cb| <= 16 h) and |t| <= reach < 2 h on every pair that reaches the test:
#   posed centre of B: three fma roundings of values <= 16 h               -> 48 u h;  t = cb - ca: one more, <= 2 u h  -> |dt| <= 50 u h
#   A's face axes:  rhs = ha + hb (Q + Q + Q), four roundings of values <= 2 h                         -> 8 u h + 50 u h  = 58 u h
#   B's face axes:  t.R, five roundings of values <= 4 h (20 u h), dt carried through sum |R| <= sqrt 3 (87 u h), rhs 8 u h  -> 115 u h
#   edge axes:      two products and a difference of values <= 4 h (12 u h), dt twice (100 u h), ra + rb seven roundings (14 u h) -> 126 u h
# so ROT_BOUND = 128 u h = 2**-17 h covers all 15; ROT_MARGIN is 128 times that (64 times is asked for).
ROT_BOUND = 128.0 * 2.0 ** -24

# axis k: (log2 res_b, rel's rotation (float32 values, row-major), t that axis k alone separates, t of the twin that overlaps);
# from a seeded random search over rotations and directions near axis k
BOX_ROT = {
    0: (-11, [0.38901209831237793, -0.6552677750587463, -0.6475289463996887, -0.5021052360534668, 0.43850237131118774, -0.7453898191452026, 0.7723729014396667, 0.6150933504104614, -0.15843066573143005],
        [0.0006678815116174519, 0.00015814696962479502, 2.7907117328140885e-06], [0.0006545511423610151, 0.0001549904845887795, 2.735011548793409e-06]),
    1: (-10, [-0.5454071760177612, 0.16139809787273407, 0.822485089302063, 0.6162363290786743, 0.7423630356788635, 0.2629636824131012, -0.5681406855583191, 0.6502674221992493, -0.5043494701385498],
        [0.00021895358804613352, 0.0010536056943237782, -4.56754096376244e-05], [0.00021441704302560538, 0.001031775726005435, -4.472905129659921e-05]),
    2: (-11, [0.8943889737129211, -0.38880640268325806, 0.22112879157066345, -0.10077401250600815, -0.6568219661712646, -0.7472814321517944, 0.4357900321483612, 0.6460762023925781, -0.6266359090805054],
        [-8.798804628895596e-05, -9.38110169954598e-05, 0.000677536241710186], [-8.553024963475764e-05, -9.119055903283879e-05, 0.0006586103700101376]),
    3: (-10, [-0.5605512261390686, -0.8062958717346191, -0.1888631135225296, -0.4588581919670105, 0.4922652840614319, -0.7396783232688904, 0.689370334148407, -0.32796621322631836, -0.6459153890609741],
        [-0.000546592811588198, -0.0003772238560486585, 0.0007322645979002118], [-0.0005008095758967102, -0.0003456271078903228, 0.0006709292065352201]),
    4: (-11, [-0.5095244646072388, 0.33430856466293335, 0.7928572297096252, 0.020888879895210266, -0.9163608551025391, 0.39980801939964294, 0.8602025508880615, 0.22027386724948883, 0.45992496609687805],
        [0.0001342065806966275, -0.0005466972943395376, 0.0003132900455966592], [0.0001311499800067395, -0.0005342460353858769, 0.0003061547176912427]),
    5: (-10, [-0.39410218596458435, -0.4623362720012665, -0.7943101525306702, -0.8634518384933472, 0.48233580589294434, 0.1476588249206543, 0.3148562014102936, 0.7440412044525146, -0.5892947316169739],
        [-0.0006023524329066277, 3.030511288670823e-05, -0.0006782063283026218], [-0.000586029898840934, 2.9483906473615207e-05, -0.000659828307107091]),
    6: (-11, [-0.12160611897706985, -0.53883296251297, 0.8335892558097839, -0.5633311867713928, 0.7289286255836487, 0.3890000283718109, -0.8172330856323242, -0.42228201031684875, -0.3921836018562317],
        [0.0002209641970694065, 0.0005845623672939837, -0.00043029244989156723], [0.0002054092474281788, 0.0005434116465039551, -0.00040000167791731656]),
    7: (-10, [0.5701202154159546, -0.36432138085365295, -0.7363646626472473, -0.6604641079902649, 0.32982540130615234, -0.6745386123657227, 0.4886206090450287, 0.8709105253219604, -0.0525810569524765],
        [-8.371283911401406e-05, -0.0009704292169772089, 0.00043911446118727326], [-7.841671322239563e-05, -0.0009090346866287291, 0.00041133371996693313]),
    8: (-11, [0.6581384539604187, 0.5503461360931396, 0.5137829184532166, 0.4604150652885437, -0.834131121635437, 0.3037157952785492, 0.5957111120223999, 0.0366663783788681, -0.8023613691329956],
        [0.00014300362090580165, 0.0005352069274522364, 0.0004978055949322879], [0.00013861895422451198, 0.0005187968490645289, 0.0004825422365684062]),
    9: (-10, [0.9516019821166992, -0.2943820059299469, -0.08827728778123856, 0.13460195064544678, 0.14098505675792694, 0.9808188080787659, -0.27628961205482483, -0.9452314376831055, 0.17378605902194977],
        [-0.0006232872256077826, -0.00039454884245060384, -0.0007213159697130322], [-0.0006127834203653038, -0.00038789978134445846, -0.0007091601146385074]),
    10: (-11, [-0.49367502331733704, 0.847551167011261, -0.19478707015514374, -0.41360291838645935, -0.425856351852417, -0.8047229051589966, -0.7649951577186584, -0.3167071044445038, 0.5607842803001404],
         [-0.000439158029621467, 0.0002346351684536785, -0.0005669055972248316], [-0.0004106585693079978, 0.0002194083499489352, -0.0005301159108057618]),
    11: (-10, [0.7686711549758911, -0.6358079314231873, -0.06994941830635071, 0.6382442712783813, 0.7696199417114258, 0.01814872771501541, 0.042295362800359726, -0.05859522148966789, 0.9973854422569275],
         [0.0009448326891288161, -1.0097748599946499e-05, 0.00026734554558061063], [0.0009282755199819803, -9.920796401274856e-06, 0.00026266061468049884]),
    12: (-11, [-0.5646480917930603, 0.7244807481765747, 0.3953482210636139, -0.7612969279289246, -0.6421937942504883, 0.08952163904905319, 0.3187468647956848, -0.2504291534423828, 0.9141584634780884],
         [0.0005637246649712324, -0.00037598542985506356, 0.00022855549468658864], [0.0005322163342498243, -0.00035497042699716985, 0.00021578081941697747]),
    13: (-10, [0.6211905479431152, -0.07748901098966599, 0.7798190116882324, 0.47300979495048523, 0.8304617404937744, -0.29427027702331543, -0.6248071789741516, 0.5516600012779236, 0.5525280833244324],
         [-0.0009446455514989793, -0.00028378565912134945, 3.182876389473677e-05], [-0.0009292661561630666, -0.00027916545514017344, 3.131057383143343e-05]),
    14: (-11, [0.22801628708839417, 0.6027024984359741, -0.76469486951828, 0.6151084303855896, -0.6979754567146301, -0.36670416593551636, -0.7547517418861389, -0.38675573468208313, -0.5298771262168884],
         [0.00022980081848800182, -0.0006324907881207764, 0.00013003405183553696], [0.00022363339667208493, -0.0006155159207992256, 0.00012654418242163956]),
}


class CubePair:
    """cube ka of A (edge RES_A) against cube kb of B (edge res_b) under rel (4x4 float32: B's frame -> A's frame)"""

    def __init__(self, name, cls, ka, kb, res_b, rel, verdict, minus=None, exact=True, sole=None):
        self.name, self.cls, self.verdict, self.minus, self.exact, self.sole = name, cls, bool(verdict), minus, exact, sole
        self.ka, self.kb = np.asarray(ka, dtype=np.int64), np.asarray(kb, dtype=np.int64)
        self.res_b, self.rel = float(res_b), np.asarray(rel, dtype=np.float32).reshape(4, 4)
        assert self.res_b in (2.0 ** -11, 2.0 ** -10)

    def t(self):
        return cloud_t(self.ka[None], RES_A, self.kb[None], self.res_b, self.rel)[0, 0]

    def with_minus(self):
        return [self] + ([self.minus] if self.minus is not None else [])


def _rel_for(R, ka, kb, res_b, t):
    """rel whose rotation is R and which carries the centre of kb to the centre of ka plus t"""
    rel = np.eye(4)
    rel[:3, :3] = R
    rel[:3, 3] = centres(ka, RES_A)[0] + np.asarray(t, dtype=np.float64) - np.asarray(R, dtype=np.float64) @ centres(kb, res_b)[0]
    return rel


def _sp_rot(perm, signs):
    R = np.zeros((3, 3))
    for r in range(3):
        R[r, perm[r]] = signs[r]
    return R


ALIGNED_RELS = [((1, 2, 0), (1, 1, 1)), ((1, 0, 2), (-1, 1, 1)), ((0, 2, 1), (1, 1, 1)), ((2, 1, 0), (-1, -1, 1))]   # two proper, two not
KA0, KB0 = (1, -2, 0), (-1, 0, 2)
K_MAX, K_MIN = (32767, -32768, 32767), (-32768, 32767, -32768)


def cube_aligned():
    """aligned cubes at equal and 2:1 resolutions: identical, face / edge / corner contact and each half a fine step apart, the small
    cube inside the large one; keys at the int16 limits.  t in units of ha = RES_A / 2: every value is exact."""
    out = []
    ha = RES_A / 2.0
    for n, (perm, signs) in enumerate(ALIGNED_RELS):
        R = _sp_rot(perm, signs)
        proper = np.linalg.det(R) > 0
        for res_b in (2.0 ** -11, 2.0 ** -10):
            h = 2 if res_b == RES_A else 3
            tag = f'{"eq" if h == 2 else "2to1"}_rel{n}'
            sx = -1 if n % 2 else 1
            plan = [('face', (sx * h, 0, 0), (sx * (h + 1), 0, 0)), ('face_y', (0, -sx * h, 0), (0, -sx * (h + 1), 0)),
                    ('edge', (h, sx * h, 0), (h, sx * (h + 1), 0)), ('edge_yz', (0, h, -h), (0, h + 1, -h)),
                    ('corner', (sx * h, h, -h), (sx * h, h, -(h + 1))), ('corner_x', (h, h, h), (h + 1, h, h))]
            plan.append(('identical', (0, 0, 0), None) if h == 2 else ('inside', (1, -1, 0), None))
            for kind, t, tm in plan:
                for ka, kb, lim in ((KA0, KB0, ''), (K_MAX, K_MIN, '_int16')):
                    if lim and kind not in ('face', 'corner'):
                        continue
                    mk = lambda tt: exact32(_rel_for(R, ka, kb, res_b, np.array(tt) * ha))
                    if tm is not None:
                        minus = CubePair(f'{kind}_{tag}{lim}_apart', 'aligned' + lim, ka, kb, res_b, mk(tm), False)
                    else:                                      # an overlapping pair: the minus variant takes B's cube three keys away
                        minus = CubePair(f'{kind}_{tag}{lim}_away', 'aligned' + lim, ka, np.array(kb) + [3, 0, 0], res_b, mk(t), False)
                    c = CubePair(f'{kind}_{tag}{lim}', 'aligned' + lim, ka, kb, res_b, mk(t), True, minus)
                    c.proper = c.minus.proper = proper
                    out.append(c)
    return out


def cube_rotated():
    """for each of the 15 axes: the twin that overlaps (True); its minus is the pair that this axis alone separates"""
    out = []
    for k, (lb, R, ts, tt) in BOX_ROT.items():
        R = np.array(R, dtype=np.float32).reshape(3, 3)
        res_b = 2.0 ** lb
        mk = lambda t: _rel_for(R, KA0, KB0, res_b, t).astype(np.float32)
        minus = CubePair(f'rot_axis{k}_separated', 'rotated', KA0, KB0, res_b, mk(ts), False, exact=False, sole=k)
        c = CubePair(f'rot_axis{k}', 'rotated', KA0, KB0, res_b, mk(tt), True, minus, exact=False, sole=k)
        c.proper = c.minus.proper = True
        h = 0.5 * (RES_A + res_b)
        for p in (c, minus):
            chain = np.abs(p.rel[:3, 3].astype(np.float64)) + np.abs(p.rel[:3, :3].astype(np.float64)) @ np.abs(centres(p.kb, res_b)[0])
            assert chain.max() <= 16 * h and np.abs(centres(p.ka, RES_A)).max() <= 16 * h
        out.append(c)
    return out


def cube_catalogue():
    return _once('cc', lambda: cube_aligned() + cube_rotated())


# ---------------------------------------------------------------------------------------------------------------------------------
# cloud scenes
class CloudScene:
    def __init__(self, name, cls, keys_a, keys_b, res_b, rel, verdict, wit=None, minus=None, pair=None, n_partner=0, res_a=RES_A):
        self.name, self.cls, self.verdict, self.wit, self.minus, self.pair, self.n_partner = name, cls, bool(verdict), wit, minus, pair, n_partner
        self.keys_a, self.keys_b = np.asarray(keys_a, dtype=np.int64).reshape(-1, 3), np.asarray(keys_b, dtype=np.int64).reshape(-1, 3)
        for k in (self.keys_a, self.keys_b):
            assert k.min() >= -32768 and k.max() <= 32767 and len(np.unique(k, axis=0)) == len(k), name
        self.res_a, self.res_b, self.rel = float(res_a), float(res_b), np.asarray(rel, dtype=np.float32).reshape(4, 4)
        self.capped = launch(len(self.keys_a), len(self.keys_b))[2] >= 2

    @property
    def shape(self):
        return len(self.keys_a), len(self.keys_b)

    def keys4(self, side):
        k = self.keys_a if side == 0 else self.keys_b
        out = np.zeros((len(k), 4), dtype=np.int16); out[:, :3] = k
        return out

    def with_minus(self):
        return [self] + ([self.minus] if self.minus is not None else [])


A_BASE, A_STEP = np.array([40, 40, 40]), 12            # A's fillers: every 12th key from (40, 40, 40): no cube of B reaches two of them
FAR_A = np.array([3000.0, 0.0, 0.0])                   # B's unpartnered fillers surround the image of this point of A's key space


def _partners(a_keys, res_b, rel):
    """for each key of A a key of B whose cube passes the reach reject against it and is separated from it by a clear margin"""
    inv = np.linalg.inv(rel.astype(np.float64))
    h = 0.5 * (RES_A + res_b)
    reach = float(reach_of(RES_A, res_b))
    off = np.array(list(itertools.product(range(-3, 4), repeat=3)))
    a_keys = np.asarray(a_keys, dtype=np.int64).reshape(-1, 3)
    if not len(a_keys):
        return []
    c = centres(a_keys, RES_A) @ inv[:3, :3].T + inv[:3, 3]
    cand = np.round(c / res_b - 0.5).astype(np.int64)[:, None, :] + off[None]                      # (n,343,3)
    r64 = rel.astype(np.float64)
    t = centres(cand.reshape(-1, 3), res_b) @ r64[:3, :3].T + r64[:3, 3] - np.repeat(centres(a_keys, RES_A), len(off), axis=0)
    e = box_axes(t, 0.5 * RES_A, 0.5 * res_b, rel[:3, :3], dtype=np.float64)
    ok = (np.all(np.abs(t) <= 0.98 * reach, axis=1) & (e.max(axis=1) >= 16 * ROT_MARGIN * h)).reshape(len(a_keys), len(off))
    return [cand[i, np.nonzero(ok[i])[0][0]] if ok[i].any() else None for i in range(len(a_keys))]


def cloud_scene(pair, na=1, nb=1, ia=0, ib=0, cls=None, name=None):
    """`pair` as key ia of A and key ib of B.  Filler c of B is a partner of filler c of A (inside `reach`, separated) while both exist;
    the rest of B's fillers, and all of them in a capped shape, lie far off."""
    capped = launch(na, nb)[2] >= 2
    rel, res_b = pair.rel, pair.res_b
    fa = A_BASE[None] + (_cells(na - 1, 16 if capped else 8) // 8) * A_STEP
    n_pair = 0 if capped else min(na - 1, nb - 1)
    fb = [p for p in _partners(fa[:n_pair], res_b, rel) if p is not None]
    n_partner = len(fb)
    inv = np.linalg.inv(rel.astype(np.float64))
    c = np.round((inv[:3, :3] @ ((FAR_A + 0.5) * RES_A) + inv[:3, 3]) / res_b).astype(np.int64)
    far = c[None] + (_cells(nb - 1 - n_partner, 40) // 8) * 2 - 40
    fb = np.concatenate([np.array(fb, dtype=np.int64).reshape(-1, 3), far])
    keys_a = np.insert(fa, ia, pair.ka, axis=0); keys_b = np.insert(fb, ib, pair.kb, axis=0)
    name = name or f'{pair.name}_{na}x{nb}_at{ia}_{ib}'
    minus = cloud_scene(pair.minus, na, nb, ia, ib, cls, name + '_minus') if pair.minus is not None else None
    s = CloudScene(name, cls or pair.cls, keys_a, keys_b, res_b, rel, pair.verdict, (ia, ib) if pair.verdict else None, minus, pair,
                   n_partner)
    s.at = (ia, ib)
    return s


def cloud_self_scene(n=1025):
    k = A_BASE[None] + (_cells(n, 16) // 8) * 2
    rel = np.eye(4, dtype=np.float32)
    return CloudScene(f'cloud_self_{n}', 'all-pairs', k, k, RES_A, rel, True)


def _cube(name):
    return {p.name: p for p in cube_catalogue()}[name]


TRAVERSAL_CUBES = ('corner_2to1_rel0', 'edge_2to1_rel2', 'rot_axis6')


def cloud_traversal_scenes():
    return _once('ct', lambda: [cloud_scene(_cube(TRAVERSAL_CUBES[i % 3]), na, nb, ia, ib, cls='traversal')
                                for i, (na, ia, nb, ib) in enumerate(traversal_positions())])


def cloud_capped_scenes():
    return _once('ccap', lambda: [cloud_scene(_cube(TRAVERSAL_CUBES[i % 2]), na, nb, ia, ib, cls='capped')
                                  for i, (na, ia, nb, ib) in enumerate(capped_positions())])


def cloud_catalogue_scenes(embedded=False):
    if embedded:
        return _once('ce', lambda: [cloud_scene(p, *EMBED) for p in cube_catalogue() if 'int16' not in p.cls])
    return _once('c1', lambda: [cloud_scene(p) for p in cube_catalogue()])
