"""Constructed scenes for the grasp filter's voxel and triangle traversal (numpy only, no GPU).

Every colliding evaluation of a case has ONE witness: a single (voxel, triangle) pair that touches.  `Case.variant(minus=True)` is the same
case without that voxel; its expected result is "free" or the next outcome of the nudge loop.  A fault of the traversal that drops part of
the work -- a block of 64 keys, a bmask word, a queue entry, a triangle chunk, a segment row -- changes a code of some case.

Expected values come from the construction, checked with float64 point-triangle distances (tests/test_collision_scenes_cpu.py), never from a
separating-axis test:
  * a witness voxel has its centre ON its triangle (exactly, for the lattice poses), and the centre is at least RES/4 away from every edge of
    the triangle in its plane (`MARGIN_CENTRE`);
  * group E (nudge loop): a triangle of edge <= 0.4 mm, small against the 1 mm nudge step, cannot hold a circle of radius RES/4 (that needs
    an edge of 0.423 mm), so there the triangle reaches RES/4 past the centre along both lattice axes of its plane and the centre is RES/8
    clear of every edge; the
    nudged poses (steps 0.001f, 0.002f are not dyadic) leave the voxel centre within 0.1 RES of the triangle's plane, the triangle being
    perpendicular to the nudge direction;
  * group F (scaled gripper_in_grasp): the voxel touches by ONE corner that penetrates the triangle's plane by RES/8, certified in float64;
  * every other (voxel, triangle) pair that the filter can form is at least RES*sqrt(3)/2 + RES apart.
So no verdict sits in a float32 rounding band.

Coordinates: RES = 2**-11; all lattice cases use poses that are pure translations by multiples of RES/8 and mesh vertices on the same
lattice, so voxel centres, translations and posed triangles are exact float32 numbers.  A mesh-frame lattice point p (in units of RES)
is the centre of the voxel with key KT + off + p for the pose of offset `off`.

Key order: `Case.keys[side]` is the STATED order in which the keys are handed to the kernel (not Morton order); `block_boxes` gives the
(lo, hi) box of every run of 64 of that order."""
import numpy as np

RES = 2.0 ** -11
U = RES / 8.0                                   # the lattice of the mesh vertices
KT = np.array([100, -60, 600], dtype=np.int64)  # key of the voxel whose centre is the mesh frame's origin at pose offset 0
I4 = np.eye(4)
R_TOUCH = RES * np.sqrt(3.0) / 2.0              # a leaf box that touches a triangle has its centre within this distance of it
FAR = R_TOUCH + RES                             # every non-witness pair is at least this far apart
MARGIN_CENTRE = RES / 4.0
TRY_OFFSETS = [(0.0, 1.0), (0.001, 1.0), (0.001, -1.0), (0.002, 1.0), (0.002, -1.0)]   # nudge index -> (step, sign) along the y column
TRY_Y = [0, 2, -2, 4, -4]                       # lattice row (units of RES) next to the triangle plane of nudge index i (1 mm = 2.048 RES)
PAIR_CAP, PAIR_DRAIN, BMASK_WORDS = 512, 256, 64


def translation(off):
    T = np.eye(4)
    T[:3, 3] = (KT + 0.5 + np.asarray(off, dtype=np.float64)) * RES
    return T


def shift(off):
    T = np.eye(4)
    T[:3, 3] = np.asarray(off, dtype=np.float64) * RES
    return T


def tri(p, shape='z'):
    """A triangle around the mesh-frame lattice point p (units of RES) -> (3,3) float64 on the RES/8 lattice."""
    p = np.asarray(p, dtype=np.float64) * RES
    if shape == 'z':          # in the plane z = p.z: edges 0.75 / 0.56 RES away from p
        d = np.array([[-8, -6, 0], [8, -6, 0], [0, 10, 0]], dtype=np.float64)
    elif shape == 'y':        # in the plane y = p.y, edges 0.366 / 0.356 / 0.356 mm
        d = np.array([[-3, 0, -2], [3, 0, -2], [0, 0, 3]], dtype=np.float64)
    elif shape == 'n111':     # normal (1,1,1), centroid p, edge 4.2 RES
        d = 8.0 * np.array([[2, -1, -1], [-1, 2, -1], [-1, -1, 2]], dtype=np.float64)
    elif shape == 'point':    # zero area
        d = np.zeros((3, 3))
    else:
        raise ValueError(shape)
    return p + d * U


def mesh_of(tris):
    V = np.concatenate([np.asarray(t, dtype=np.float64).reshape(3, 3) for t in tris])
    return V, np.arange(len(V), dtype=np.int32).reshape(-1, 3)


def block_boxes(keys):
    """(n,3) keys in stated order -> (ceil(n/64), 2, 3): lowest / highest key of every run of 64 (the last run may be partial)."""
    keys = np.asarray(keys, dtype=np.int64).reshape(-1, 3)
    nb = (len(keys) + 63) // 64
    out = np.zeros((nb, 2, 3), dtype=np.int64)
    for b in range(nb):
        run = keys[b * 64:(b + 1) * 64]
        out[b, 0] = run.min(axis=0); out[b, 1] = run.max(axis=0)
    return out


def f32(x):
    return np.float32(x)


def tried_translation(t, idx):
    """The float32 translation of nudge index idx for a pose of identity rotation and translation t (common.cpp:265)."""
    sign = TRY_OFFSETS[idx][1]
    st = f32(0.0) if idx == 0 else (f32(0.001) if idx < 3 else f32(f32(0.001) + f32(0.001)))
    t = np.asarray(t, dtype=np.float32).copy()
    for r, major in enumerate((0.0, 1.0, 0.0)):
        t[r] = f32(t[r] + f32(f32(st * f32(major)) * f32(sign)))
    return t


class Case:
    """One constructed scene.  tris[s] / keys[s]: the mesh and the stated-order voxel keys of side s (0: open gripper vs the object's voxels,
    1: enclosed gripper vs the background).  hits[e] = {nudge index: side} names the tried poses of evaluation e at which a witness touches;
    wit = (side, key index, e, nudge index) is the witness that the minus variant removes."""

    def __init__(self, name, group, tris, keys, hits, wit, poses=None, syms=None, gig=None, adjust=0, stats=False, corner=None,
                 routes='all', note=''):
        self.name, self.group, self.adjust, self.stats, self.routes, self.note = name, group, int(adjust), stats, routes, note
        self.tris = [np.asarray(t, dtype=np.float64).reshape(-1, 3, 3) for t in tris]
        self.keys = [np.asarray(k, dtype=np.int64).reshape(-1, 3) for k in keys]
        self.poses = np.asarray(poses if poses is not None else [translation((0, 0, 0)), translation((0, 0, 8))], dtype=np.float64)
        self.syms = np.asarray(syms if syms is not None else [I4], dtype=np.float64)
        self.gig = np.asarray(gig if gig is not None else I4, dtype=np.float64)
        self.hits, self.wit, self.corner = hits, wit, corner
        self.res = RES
        self.minus = False
        for k in self.keys:
            assert len(k) == 0 or (k.min() >= -32768 and k.max() <= 32767), name
            assert len(np.unique(k, axis=0)) == len(k), f'{name}: duplicate keys'

    # ---- the inputs
    def mesh(self, side):
        return mesh_of(self.tris[side])

    def points(self, side):
        """voxel centres (exact float32) in stated order; the far sentinel of generate_grasp.py for an empty set"""
        k = self.keys[side]
        return ((k + 0.5) * RES).astype(np.float32) if len(k) else np.full((1, 3), 99999.0, dtype=np.float32)

    def boxes(self, side):
        return block_boxes(self.keys[side])

    @property
    def E(self):
        return len(self.poses) * len(self.syms)

    def gic(self):
        """grasp_in_cam of every evaluation (translations only, exact in float32) -> (E,4,4) float32"""
        out = np.zeros((self.E, 4, 4), dtype=np.float32)
        for i, P in enumerate(self.poses):
            for j, S in enumerate(self.syms):
                out[i * len(self.syms) + j] = (S @ P).astype(np.float32)
        return out

    def variant(self, minus=False, adjust=None, first_eval_only=False):
        """the same case without its witness voxel (minus), with another adjust flag, or cut down to its first evaluation"""
        import copy
        c = copy.copy(self)
        c.keys = [k.copy() for k in self.keys]
        c.hits = {e: dict(h) for e, h in self.hits.items()}
        if minus:
            assert self.wit is not None and not self.minus
            s, i, e, ti = self.wit
            c.keys[s] = np.delete(c.keys[s], i, axis=0)
            del c.hits[e][ti]
            c.wit, c.corner, c.minus = None, None, True
        if adjust is not None:
            c.adjust = int(adjust)
        if first_eval_only:
            c.poses, c.syms = self.poses[:1], self.syms[:1]
            c.hits = {e: h for e, h in c.hits.items() if e == 0}
        return c

    # ---- the expected outputs, from the construction
    def expected(self, keep_rejected_pose=False):
        """-> codes (E) int8, poses (E,4,4) float32, nudge (E) int8"""
        gic = self.gic()
        codes = np.zeros(self.E, dtype=np.int8); nudge = np.full(self.E, -1, dtype=np.int8); poses = np.zeros_like(gic)
        for e in range(self.E):
            h = self.hits.get(e, {})
            if not self.adjust:
                if 0 in h:
                    codes[e] = 3 + h[0]
                else:
                    nudge[e] = 0
            else:
                free = [i for i in range(5) if i not in h]
                if free:
                    nudge[e] = free[0]
                else:
                    codes[e] = 3
            if codes[e] == 0:
                poses[e] = gic[e]
                poses[e, :3, 3] = tried_translation(gic[e, :3, 3], int(nudge[e]))
            elif keep_rejected_pose:
                poses[e] = gic[e]
        return codes, poses, nudge


# ---------------------------------------------------------------------------------------------------------------------------------
# float64 geometry
def point_tri_dist(P, T):
    """P (n,3), T (m,3,3) -> (distance (n,m), distance to the nearest EDGE (n,m)) in float64; zero-area triangles are their edges."""
    P = np.asarray(P, dtype=np.float64); T = np.asarray(T, dtype=np.float64)
    a, b, c = T[:, 0], T[:, 1], T[:, 2]

    def seg(u, v):
        uv = v - u
        l2 = (uv * uv).sum(-1)
        up = P[:, None, :] - u[None]
        t = np.clip(np.where(l2 > 0, (up * uv[None]).sum(-1) / np.where(l2 > 0, l2, 1.0), 0.0), 0.0, 1.0)
        return np.linalg.norm(up - t[..., None] * uv[None], axis=-1)
    dseg = np.minimum(np.minimum(seg(a, b), seg(b, c)), seg(c, a))
    n = np.cross(b - a, c - a)
    nn = np.linalg.norm(n, axis=-1)
    ok = nn > 0
    nh = n / np.where(ok, nn, 1.0)[:, None]
    dpl = ((P[:, None, :] - a[None]) * nh[None]).sum(-1)
    q = P[:, None, :] - dpl[..., None] * nh[None]

    def side(u, v):
        return (np.cross((v - u)[None], q - u[None]) * nh[None]).sum(-1)
    inside = ok[None] & (side(a, b) >= 0) & (side(b, c) >= 0) & (side(c, a) >= 0)
    return np.where(inside, np.abs(dpl), dseg), dseg


def posed_tris(case, side, e, idx):
    """float64 triangles of mesh `side` as the filter poses them for evaluation e at nudge index idx (float32 pose entries)"""
    t = tried_translation(case.gic()[e, :3, 3], idx).astype(np.float64)
    g = case.gig.astype(np.float32).astype(np.float64)
    assert np.all(g[:3, 3] == 0) and np.all(g[:3, :3] == np.diag(np.diag(g[:3, :3])))
    return case.tris[side] * np.diag(g[:3, :3])[None, None, :] + t[None, None, :], np.diag(g[:3, :3]).copy(), t


def tries(case):
    return range(5) if case.adjust else range(1)


def corner_penetration(centre, T):
    """leaf box of half edge RES/2 at `centre` against the plane of triangle T (3,3): -> (depth of the deepest corner past the plane,
    depth of the second deepest, in-plane clearance of the deepest corner's projection from the triangle's edges)"""
    n = np.cross(T[1] - T[0], T[2] - T[0]); n /= np.linalg.norm(n)
    if np.dot(np.asarray(centre) - T[0], n) > 0:
        n = -n                                              # the box lies on the -n side; corners poke through towards +n
    corners = np.asarray(centre)[None] + 0.5 * RES * np.array([[sx, sy, sz] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)])
    depth = (corners - T[0]) @ n
    o = np.argsort(-depth)
    q = corners[o[0]] - depth[o[0]] * n
    _, edge = point_tri_dist(q[None], T[None])
    d, _ = point_tri_dist(q[None], T[None])
    return depth[o[0]], depth[o[1]], (edge[0, 0] if d[0, 0] < 1e-12 else -1.0)


# ---------------------------------------------------------------------------------------------------------------------------------
# numpy restatement of the grid kernel's traversal (MeshGrid's numbers, relevant_blocks, the voxel passes and the pair queue)
def grid_params(V, F, res):
    V = np.asarray(V, dtype=np.float64)
    inflate = 2.0 * (res * np.sqrt(3.0) / 2.0) + 3e-5
    cell = max(2.0 * res, 0.001) if len(F) >= 2000 else max(4.0 * res, 0.002)
    lo = V.min(axis=0) - inflate - 1e-6
    hi = V.max(axis=0) + inflate + 1e-6
    dims = np.maximum(np.ceil((hi - lo) / cell).astype(np.int64), 1)
    return lo, dims, cell, inflate


def grid_lists(case, side):
    from catgrasp_amd.my_cpp import MeshGrid
    V, F = case.mesh(side)
    V = V.astype(np.float32).astype(np.float64)
    lo, dims, cell, inflate = grid_params(V, F, RES)
    start, tids = MeshGrid._host_lists(V, F.astype(np.int64), lo, dims, cell, inflate, int(np.prod(dims)))
    return dict(lo=lo, dims=dims, cell=cell, inflate=inflate, start=start.astype(np.int64), tids=tids, V=V, F=F)


def traversal(case, side, use_blocks=True, g=None):
    """What the grid kernel does for evaluation 0 at nudge index 0 against the keys of `side`, when nothing collides:
    -> dict(visited (block ids), work0 (keys read), work1 (cells looked up), work2 (pairs queued), cnt (list length per key),
            border (smallest distance of a key's grid coordinate from a cell border, in cells), robust (the block decisions do not depend
            on the slack), flushes (queue fills at every test), midpass (a flush with lists still to queue), slot (queue position of
            every pair as (key index, triangle) -> (flush number, slot)))"""
    g = g or grid_lists(case, side)
    _, s, t = posed_tris(case, side, 0, 0)
    keys = case.keys[side]
    nk = len(keys)
    lo, dims, cell, start = g['lo'], g['dims'], g['cell'], g['start']
    A = RES / (s * cell)                                            # key -> grid coordinate, per axis (diagonal poses)
    b = ((0.5 * RES - t) / s - lo) / cell
    f = keys * A[None] + b[None]
    inb = np.all((f >= 0) & (f < dims[None]), axis=1)
    ci = np.floor(np.where(inb[:, None], f, 0)).astype(np.int64)
    cid = (ci[:, 0] * dims[1] + ci[:, 1]) * dims[2] + ci[:, 2]
    cnt = np.where(inb, start[cid + 1] - start[cid], 0)
    near = f[np.all((f > -1) & (f < dims[None] + 1), axis=1)]
    border = float(np.abs(near - np.round(near)).min()) if len(near) else 1.0
    nb = (nk + 63) // 64
    ne = (start[1:] != start[:-1]).reshape(dims)
    sd = (dims + 3) // 4
    coarse = np.zeros(sd, dtype=bool)
    ix, iy, iz = np.nonzero(ne)
    coarse[ix // 4, iy // 4, iz // 4] = True

    def keep(slack):
        out = np.ones(nb, dtype=bool)
        if not use_blocks:
            return out
        bx = case.boxes(side)
        for blk in range(min(nb, BMASK_WORDS * 64)):
            c = 0.5 * (bx[blk, 0] + bx[blk, 1]); h = 0.5 * (bx[blk, 1] - bx[blk, 0])
            fc = A * c + b; rad = np.abs(A) * h + slack
            f0, f1 = fc - rad, fc + rad
            if np.any(f1 < 0) or np.any(f0 >= dims):
                out[blk] = False
                continue
            c0 = np.where(f0 > 0, np.floor(np.maximum(f0, 0)), 0).astype(np.int64) >> 2
            c1 = np.where(f1 < dims - 1, np.floor(np.minimum(f1, dims - 1)), dims - 1).astype(np.int64) >> 2
            if np.all(c1 - c0 <= 2):
                out[blk] = coarse[c0[0]:c1[0] + 1, c0[1]:c1[1] + 1, c0[2]:c1[2] + 1].any()
        return out
    kp = keep(1e-3)
    robust = bool(np.array_equal(kp, keep(0.0)) and np.array_equal(kp, keep(1e-2)))
    visited = np.nonzero(kp)[0]
    read = np.zeros(nk, dtype=bool)
    for blk in visited:
        read[blk * 64:(blk + 1) * 64] = True
    # the passes (two visited blocks each) and the queue
    fill, flushes, midpass, slot = 0, [], False, {}
    tids = g['tids']
    for p0 in range(0, len(visited), 2):
        lanes = []
        for lane in range(64):
            ent = []
            for blk in visited[p0:p0 + 2]:
                v = blk * 64 + lane
                if v < nk and inb[v]:
                    ent += [(v, int(tt)) for tt in tids[start[cid[v]]:start[cid[v] + 1]]]
            lanes.append(ent)
        r = 0
        while True:
            act = [ln for ln in range(64) if len(lanes[ln]) > r]
            if act and fill + 64 <= PAIR_CAP:
                for q, ln in enumerate(act):
                    slot[lanes[ln][r]] = (len(flushes), fill + q)
                fill += len(act); r += 1
                continue
            if fill and (act or fill >= PAIR_DRAIN):
                flushes.append(fill); midpass |= bool(act); fill = 0
            if not act:
                break
    if fill:
        flushes.append(fill)
    return dict(visited=visited, work0=int(read.sum()), work1=int((read & inb).sum()), work2=int(cnt[read].sum()), cnt=cnt, border=border,
                robust=robust, flushes=flushes, midpass=midpass, slot=slot, nblocks=nb, grid=g)


# ---------------------------------------------------------------------------------------------------------------------------------
# the cases
DECOY = (60, 60, 60)          # a second small triangle that gives the mesh grid 16 cells per axis
DUMMY = [tri((90, 90, 90))]   # the mesh of the side that a case does not use
COMPANION = [4, 0, 0]         # a lattice point 3 RES from the 'z' triangle at the origin, in a cell that lists it


def _sides(side, main_tris, main_keys):
    tris = [DUMMY, DUMMY]; keys = [np.zeros((0, 3), dtype=np.int64)] * 2
    tris[side] = main_tris; keys[side] = np.asarray(main_keys, dtype=np.int64)
    return tris, keys


def _simple(name, group, side, tris, pts, wi, **kw):
    """mesh-frame lattice points pts (stated order, witness at index wi, touching at evaluation 0 / nudge index 0) on `side`"""
    off = kw.pop('kt_off', np.zeros(3, dtype=np.int64))
    keys = KT + off + np.asarray(pts, dtype=np.int64)
    t, k = _sides(side, tris, keys)
    if 'poses' not in kw:
        kw['poses'] = [translation(off), translation(off + np.array([0, 0, 8]))]
    return Case(name, group, t, k, {0: {0: side}}, (side, wi, 0, 0), **kw)


def _far_a(n):
    """n lattice points well away from the witness triangle (origin) and from the decoys (positive octant)"""
    i = np.arange(n)
    return np.stack([i % 8, -24 - (i // 8) % 8, -(i // 64)], axis=1)


def _group_a():
    cases = []
    nks = [(1, 'first'), (63, 'first'), (64, 'last'), (65, 'first'), (129, 'last'), (1, 'last'), (63, 'last'), (64, 'first'), (65, 'last'),
           (129, 'first')]
    spots = [(16 * (1 + a), 16 * (1 + b), 16 * (1 + c)) for a in range(7) for b in range(7) for c in range(7)]
    n = 0

    def make(nf, wi, nk, where, shape='z', kt_off=None, tag=''):
        tris = [tri(spots[j], shape) for j in range(nf)]
        tris[wi] = tri((0, 0, 0))
        others = _far_a(nk - 1)
        pts = np.concatenate([[[0, 0, 0]], others]) if where == 'first' else np.concatenate([others, [[0, 0, 0]]])
        kw = dict(kt_off=kt_off) if kt_off is not None else {}
        return _simple(f'A_nf{nf}_w{wi}_nk{nk}_{where}{tag}', 'A', 0, tris, pts, 0 if where == 'first' else nk - 1, **kw)
    for nf in (1, 63, 64, 65, 128, 129, 130, 257):
        for wi in sorted({i for i in (0, 63, 64, 127, 128, 129, nf - 1) if i < nf}):
            nk, where = nks[n % len(nks)]; n += 1
            cases.append(make(nf, wi, nk, where))
    cases.append(make(130, 129, 65, 'last', shape='point', tag='_degenerate'))
    cases.append(make(65, 64, 65, 'first', kt_off=np.array([-32768, 32767, 0]) - KT, tag='_keymin'))
    return cases


def _b_others(n):
    i = np.arange(n)
    return np.stack([16 + i // 512, 16 + (i // 32) % 16, 8 + i % 32], axis=1)


def _group_b():
    cases = []
    mesh = [tri((0, 0, 0)), tri(DECOY)]
    for n, q in enumerate((0, 1, 63, 64)):
        pts = np.concatenate([_b_others(64 * q), [[0, 0, 0]]])
        cases.append(_simple(f'B_last_q{q}', 'B', n % 2, mesh, pts, 64 * q, stats=True))
    for n, (blk, lane) in enumerate(((0, 0), (63, 63), (64, 31), (65, 1), (127, 62))):
        # a companion 4 voxels beside the witness, half a block away in the key order, keeps the block relevant in the minus variant
        wi, ci = blk * 64 + lane, blk * 64 + (lane + 32) % 64
        pts = np.zeros((8192, 3), dtype=np.int64)
        pts[wi], pts[ci] = [0, 0, 0], COMPANION
        pts[np.setdiff1d(np.arange(8192), [wi, ci])] = _b_others(8190)
        cases.append(_simple(f'B_block{blk}_lane{lane}', 'B', (n + 1) % 2, mesh, pts, wi, stats=True))
    i = np.arange(262144)
    cube = np.stack([-300 + i // 4096, -300 + (i // 64) % 64, -300 + i % 64], axis=1)
    row = np.stack([-100 - np.arange(64), np.full(64, -100), np.full(64, -100)], axis=1)
    pts = np.concatenate([cube, row, [[0, 0, 0]]])
    cases.append(_simple('B_beyond_table', 'B', 0, mesh, pts, len(pts) - 1, stats=True, routes='accel'))
    return cases


C_W = 64


def _c_mesh(m, where):
    top = 16 * m + 16
    decoys = [np.array([[0, 16 * j, 0], [C_W, 16 * j, C_W], [C_W, top, C_W]], dtype=np.float64) * RES for j in range(m)]
    # the witness triangle: among all m decoys' lists (last), among those of m - 1 (cap), or away from them (first)
    pw = {'last': (C_W - 4, 16 * (m - 1) + 8, 4), 'cap': (C_W - 4, 16 * (m - 2) + 8, 4), 'first': (C_W - 4, -24, 4)}[where]
    return decoys + [tri(pw)], np.array(pw)


def _group_c():
    """Queue cases: m decoys whose boxes cover a slab of voxels (lists of up to m entries, nothing near), and the witness triangle with the
    highest index.  The voxels are chosen by the list length of their cell so that the pairs queued over the set number `total`."""
    cases = []
    plan = [(t, m, w) for t, m in ((255, 1), (256, 1), (257, 1), (511, 4), (512, 4), (513, 4), (1601, 5)) for w in ('first', 'last')]
    plan += [(636, 5, 'first'), (641, 5, 'last')]      # one pass of 128 voxels queues more than PAIR_CAP pairs: the flush in mid-pass
    plan += [(512, 4, 'cap')]                          # one pass of 128 voxels with four entries each: the queue filled to PAIR_CAP exactly
    for n, (total, m, where) in enumerate(plan):
        tris, pw = _c_mesh(m, where)
        # candidates: the corner of the decoys' boxes that is far from their common plane z = x, level by level
        levels = []
        for lv in range(1, m + 1):
            y0 = 16 * (lv - 1) + 6
            y1 = y0 + 4 if lv < m else 16 * m + 12
            ys, xs, zs = np.meshgrid(np.arange(y0, y1), np.arange(C_W - 8, C_W), np.arange(0, 8), indexing='ij')
            levels.append(np.stack([xs.ravel(), ys.ravel(), zs.ravel()], axis=1))
        pool = np.concatenate(levels)
        pool = pool[np.abs(pool - pw[None]).max(axis=1) >= 8]       # two cells away from the witness triangle's lists
        probe = _simple('probe', 'C', 0, tris, np.concatenate([[pw], pool]), 0)
        cnt = traversal(probe, 0, use_blocks=False)['cnt']
        w, cnt = int(cnt[0]), cnt[1:]
        assert w == {'last': m + 1, 'cap': m, 'first': 1}[where], (w, m, where)
        need = total - w
        full = pool[cnt == m][:need // m]
        rest = pool[cnt == need % m][:1] if need % m else pool[:0]
        assert len(full) == need // m and len(rest) == (1 if need % m else 0)
        others = np.concatenate([full, rest])
        pts = np.concatenate([[pw], others]) if where == 'first' else np.concatenate([others, [pw]])
        name = f'C_pairs{total}_m{m}_{where}' + ('_onepass' if total in (636, 641) else '')
        c = _simple(name, 'C', n % 2, tris, pts, 0 if where == 'first' else len(pts) - 1, stats=True)
        c.pairs_total, c.m, c.where, c.wit_pairs = total, m, where, w
        cases.append(c)
    return cases


def _outside(n, row):
    return np.stack([-300 + np.arange(n), np.full(n, -300 - 4 * row), np.full(n, -300)], axis=1)


def _group_d():
    cases = []
    mesh = [tri((0, 0, 0)), tri(DECOY)]
    # 1: the witness block's box reaches 0.67 cells into the grid; every other block lies outside
    # (with a companion that keeps the box 0.19 cells inside along x when the witness is gone)
    line = np.stack([-9 - np.arange(62), np.zeros(62, dtype=np.int64), np.zeros(62, dtype=np.int64)], axis=1)
    wb = np.insert(np.insert(line, 20, [-2, 3, 0], axis=0), 40, [0, 0, 0], axis=0)
    pts = np.concatenate([_outside(64, 0), _outside(64, 1), wb, _outside(64, 2), _outside(64, 3)])
    cases.append(_simple('D_touch_by_less_than_a_cell', 'D', 0, mesh, pts, 128 + 40, stats=True))
    # 2: a block whose box covers the whole grid (4 coarse cells per axis: no coarse test), all keys but the witness outside
    lo = np.stack([-20 - np.arange(32), np.full(32, -20), np.full(32, -20)], axis=1)
    hi = np.stack([90 + np.arange(31), np.full(31, 90), np.full(31, 90)], axis=1)
    wb = np.concatenate([lo, [[0, 0, 0]], hi])
    pts = np.concatenate([_outside(64, 0), wb, _outside(64, 1)])
    cases.append(_simple('D_box_straddles_grid', 'D', 1, mesh, pts, 64 + 32, stats=True))
    # 3: a block inside the grid over empty coarse cells (culled), the witness in the next block over an occupied coarse cell
    i = np.arange(64)
    empty = np.stack([28 + i // 16, 28 + (i // 4) % 4, 28 + i % 4], axis=1)
    occ = np.stack([8 + i // 16, 8 + (i // 4) % 4, 8 + i % 4], axis=1)[:63]
    wb = np.insert(occ, 17, [0, 0, 0], axis=0)
    pts = np.concatenate([_outside(64, 0), empty, wb, _outside(64, 1)])
    cases.append(_simple('D_empty_coarse_neighbour', 'D', 0, mesh, pts, 128 + 17, stats=True))
    return cases


E_PW = [np.array([0, 0, 0]), np.array([24, 0, 0])]     # the witness triangles of the open and of the enclosed mesh (perpendicular to y)


def _e_case(name, present, adjust, group='E', extra=None):
    """present: {nudge index: side} -- one voxel next to the triangle of that side for each tried offset that is to collide"""
    tris = [[tri(E_PW[0], 'y'), tri(DECOY)], [tri((40, 40, 40)), tri(E_PW[1], 'y')]]
    far = [np.array([[-20, 0, 0], [-20, 9, 3], [-24, -9, 0]]), np.array([[-30, 0, 0], [-30, 9, 3]])]
    pts = [list(far[0]), list(far[1])]
    where = {}
    for idx, side in present.items():
        where[idx] = (side, len(pts[side]))
        pts[side].append(E_PW[side] + np.array([0, TRY_Y[idx], 0]))
    for side, p in (extra or []):
        pts[side].append(np.asarray(p))
    keys = [KT + np.asarray(p, dtype=np.int64) for p in pts]
    wit = None
    if present:
        # the witness the minus variant removes: the last tried offset that collides
        order = [i for i in range(5) if i in present]
        cut = order[-1] if adjust else order[0]
        wit = (where[cut][0], where[cut][1], 0, cut)
    poses = [translation((0, 0, 0))]
    syms = [I4, shift((0, 0, 16))]
    return Case(name, group, tris, keys, {0: dict(present)}, wit, poses=poses, syms=syms, adjust=adjust)


def _group_e():
    cases = []
    for side in (0, 1):
        s = 'open' if side == 0 else 'bg'
        for adjust in (0, 1):
            for n in range(6):
                present = {i: side for i in range(n)}
                cases.append(_e_case(f'E_{s}_collide{n}_adjust{adjust}', present, adjust))
    for adjust in (0, 1):
        cases.append(_e_case(f'E_mixed_open0_bg1_adjust{adjust}', {0: 0, 1: 1}, adjust))
        # a voxel of each set next to the OTHER mesh's triangle: never paired, so free
        cases.append(_e_case(f'E_cross_adjust{adjust}', {}, adjust, extra=[(0, E_PW[1]), (1, E_PW[0])]))
    return cases


def _group_f():
    cases = []
    for name, d in (('F_scale086', (0.86, 0.86, 0.86)), ('F_scale088', (0.88, 0.88, 0.88)), ('F_aniso052', (1.0, 1.0, 0.52))):
        gig = np.diag(list(d) + [1.0])
        g32 = np.diag(gig).astype(np.float32).astype(np.float64)[:3]
        T0 = tri((0, 0, 0), 'n111')
        n = np.cross((T0[1] - T0[0]) * g32, (T0[2] - T0[0]) * g32); n /= np.linalg.norm(n)
        if n.sum() < 0:
            n = -n
        kw = KT + np.array([40, 40, 40])
        c = (kw + 0.5) * RES
        q = c + 0.5 * RES * np.sign(n) - (RES / 8.0) * n           # the posed centroid: RES/8 behind the corner that pokes through
        t = q.astype(np.float32).astype(np.float64)
        P = np.eye(4); P[:3, 3] = t
        far = np.array([[-10, 0, 0], [0, -12, 0], [12, 9, 10], [20, 20, 25]])       # two outside the mesh grid, two inside
        keys = np.concatenate([kw + far[:2], [kw], kw + far[2:]])
        tr, ky = _sides(0, [T0, tri(DECOY)], keys)
        cases.append(Case(name, 'F', tr, ky, {0: {0: 0}}, (0, 2, 0, 0), poses=[P], syms=[I4], gig=gig, stats=True, corner=(0, 2, 0)))
    return cases


def build_cases():
    return _group_a() + _group_b() + _group_c() + _group_d() + _group_e() + _group_f()


_cases = None


def cases():
    global _cases
    if _cases is None:
        _cases = build_cases()
        assert len({c.name for c in _cases}) == len(_cases)
    return _cases


def case(name):
    return {c.name: c for c in cases()}[name]


# ---- group G: a segment table whose rows alternate between "has the witness" and minus, with the nudge flag alternating too
def segment_table(n_segments=2600):
    """-> (with-witness case, rows): rows[i] = (kind, n_pose, adjust) with kind in {'wit', 'minus', 'novox'}; n_pose cycles 1, 2, 3, 0.
    Every pose of a row is the witness pose, so a row's evaluations all have the row's expected result."""
    base = _e_case('G_base', {0: 0}, 0, group='G')
    rows = []
    for i in range(n_segments):
        kind = 'novox' if i % 7 == 5 else ('wit' if i % 2 == 0 else 'minus')
        rows.append((kind, (1, 2, 3, 0)[i % 4] if i % 11 else 0, (i // 2 + i // 3) % 2))
    return base, rows


def segment_expected(base, rows):
    codes, nudge, poses = [], [], []
    for kind, n, adjust in rows:
        c = base.variant(minus=(kind != 'wit'), adjust=adjust, first_eval_only=True)
        co, po, nu = c.expected()
        codes += [co[0]] * n; nudge += [nu[0]] * n; poses += [po[0]] * n
    return np.array(codes, dtype=np.int8), np.array(poses, dtype=np.float32).reshape(-1, 4, 4), np.array(nudge, dtype=np.int8)
