"""Host reference of the PointNet++ grouping primitives (csrc/primitives.hip: square_distance, square_distance_nd, index_points,
ball_query, group_points) in plain numpy float64, and the scenes tests/test_primitives_edges_gpu.py runs them on.  Proved on the CPU
by tests/test_group_ref_cpu.py.

The references state the operation itself: the squared distance is sum_c (s_c - d_c)^2, not the -2ab + a^2 + b^2 expansion; a ball
is "every point that is not farther than r^2", its row "the first nsample members by index, padded with the first"; a gather is
fancy indexing; the grouped tensor is sa_ref.grouped.  Chunks of 64, trips of 512, four queries per workgroup, prefix popcounts and
the padding loop are properties of the code under test.

Three kinds of scene:
  * exact scenes: coordinates k/64 (0 <= k < 64), features of other widths small integers over 8.  Every product of the expansion
    is a multiple of g = step^2 (2^-12, 2^-6) and while 2 sum|s d| + sum s^2 + sum d^2 stays below 2^24 g (exactness_margin < 1)
    every partial sum is a float32 number: the float32 result is the same in every order, with or without FMA, and equals the
    float64 one.  The kernels are held to equality on them, and a ball's membership has no rounding band at all;
  * planted ball scenes (exact scenes): the background lies on the lattice many steps outside every ball and a named list of hit
    indices per query is placed at lattice offsets inside it, so the expected row is known in closed form (planted_rows);
  * general-value scenes: normal clouds, held per element to sqdist_bound; for a ball query r^2 is searched among float32 numbers
    near the nominal radius until every (query, point) pair clears it by more than that bound (general_ball_scene): no membership
    can flip under any float32 evaluation within the bound, every row is held to equality and none is excused."""
import numpy as np

from sa_ref import grouped                                   # noqa: F401  (the gather + centre + concat reference, reused as it is)

U32 = 2.0 ** -24            # unit roundoff of float32
U64 = 2.0 ** -53
STEP_XYZ = 2.0 ** -6        # the exact scenes' coordinate lattice
STEP_FEAT = 2.0 ** -3       # ... and their feature lattice


# ------------------------------------------------------------------------------------------------------------ reference
def sqdist_ref(src, dst):
    """src (B,N,C), dst (B,M,C) -> (B,N,M) float64: sum_c (s_c - d_c)^2, any C."""
    s = np.asarray(src, np.float64)[:, :, None, :]
    d = np.asarray(dst, np.float64)[:, None, :, :]
    return ((s - d) ** 2).sum(axis=-1)


def gamma(k, u=U32):
    return k * u / (1.0 - k * u)


def sqdist_magnitude(src, dst):
    """2 sum_c |s_c d_c| + sum_c s_c^2 + sum_c d_c^2, (B,N,M) float64: the sum of the magnitudes of the expansion's terms."""
    s = np.asarray(src, np.float64)
    d = np.asarray(dst, np.float64)
    cross = np.abs(s) @ np.abs(d).transpose(0, 2, 1)
    return 2.0 * cross + (s * s).sum(-1)[:, :, None] + (d * d).sum(-1)[:, None, :]


def sqdist_bound(src, dst):
    """Per-element bound, (B,N,M) float64, on |v - sqdist_ref| for v = (-2 dot + |s|^2) + |d|^2 evaluated in float32 on the float32
    inputs, the three sums accumulated over the channels without FMA (pointnet2.py:30-32, and both kernels).

    Derivation from the operation count.  dot, |s|^2 and |d|^2 are each a sum of C rounded products: whatever the order of the
    additions, a product goes through its own rounding and at most C - 1 additions, C roundings (an FMA only removes one).  The
    factor -2 is exact.  The two final additions add two roundings to every term of dot and |s|^2 and one to every term of |d|^2.
    The longest chain is therefore k = C + 2 roundings, each term t is returned as t (1 + theta) with |theta| <= gamma_k, and
        |v - exact| <= gamma_k (2 sum|s_c d_c| + sum s_c^2 + sum d_c^2),     gamma_k = k u / (1 - k u),  u = 2^-24
    (Higham, Accuracy and Stability of Numerical Algorithms, lemma 3.1).  `exact` is the expansion in real arithmetic, which is
    sum (s_c - d_c)^2; the float64 evaluation of that by sqdist_ref carries C subtractions, squares and additions of its own, below
    gamma_{C+2}(2^-53) times the same magnitude sum, which is added.  Nothing here is fitted to any output."""
    C = np.asarray(src).shape[-1]
    return (gamma(C + 2, U32) + gamma(C + 2, U64)) * sqdist_magnitude(src, dst)


def ball_ref(xyz, new_xyz, r2_f32, nsample):
    """xyz (B,N,3), new_xyz (B,S,3) -> (B, S, min(nsample, N)) int64.  A point is a member of a query's ball unless its squared distance
    is greater than r^2 (so a NaN distance is a member, pointnet2.py:92); the row holds the first min(nsample, N) members in
    ascending index order, the free slots hold the first member, and an empty ball holds N everywhere.  r2_f32: the float32 number
    the comparison is made against (torch compares a float32 tensor with a Python scalar in float32)."""
    assert np.asarray(r2_f32).dtype == np.float32
    member = ~(sqdist_ref(new_xyz, xyz) > np.float64(r2_f32))
    B, S, N = member.shape
    ns = min(int(nsample), N)
    out = np.full((B, S, ns), N, np.int64)
    for b in range(B):
        for s in range(S):
            m = np.flatnonzero(member[b, s])
            if len(m):
                out[b, s] = m[0]
                out[b, s, :min(ns, len(m))] = m[:ns]
    return out


def r2_of(radius):
    """The float32 number a ball query of `radius` compares with: float32(radius ** 2), the square taken in double."""
    return np.float32(float(radius) ** 2)


def index_ref(points, idx):
    """points (B,N,C), idx (B,...) -> (B,...,C): plain fancy indexing, any dtype (bit patterns pass through an integer view)."""
    points = np.asarray(points)
    idx = np.asarray(idx)
    bi = np.arange(points.shape[0]).reshape((-1,) + (1,) * (idx.ndim - 1))
    return points[bi, idx]


def exactness_margin(src, dst, step):
    """Largest (2 sum|s d| + sum s^2 + sum d^2) / (2^24 step^2) over all (source, destination) pairs.  Inputs are multiples of `step`,
    so every product is a multiple of g = step^2; below 1 every partial sum of the expansion, in any order, is a multiple of g below
    2^24 g: exact in float32.  Raises if an input is off the lattice.  Rows holding a NaN are left out (they give NaN in any
    evaluation)."""
    keep = []
    for t in (src, dst):
        t = np.asarray(t, np.float64)
        t = np.where(np.isnan(t).any(-1, keepdims=True), 0.0, t)
        q = t / step
        assert np.array_equal(q, np.round(q)), 'input is not a multiple of the step'
        keep.append(t)
    m = sqdist_magnitude(*keep)
    return (float(m.max()) if m.size else 0.0) / (2.0 ** 24 * step * step)


# --------------------------------------------------------------------------------------------------------- exact scenes
def exact_clouds(B, N, M, C, seed):
    """-> (src (B,N,C), dst (B,M,C), step) float64: C = 3: coordinates k/64, 0 <= k < 64; other widths: integers in [-16, 16] over 8.
    Every cloud is drawn on its own, so a wrong batch offset shows."""
    rng = np.random.default_rng(seed)
    if C == 3:
        return rng.integers(0, 64, (B, N, C)) * STEP_XYZ, rng.integers(0, 64, (B, M, C)) * STEP_XYZ, STEP_XYZ
    return rng.integers(-16, 17, (B, N, C)) * STEP_FEAT, rng.integers(-16, 17, (B, M, C)) * STEP_FEAT, STEP_FEAT


def general_clouds(B, N, M, C, seed):
    """-> (src, dst) float32: C = 3: the clouds of test_primitives_gpu._cloud (sigma 0.05, z offset 0.6); other widths: unit normals."""
    rng = np.random.default_rng(seed)
    if C == 3:
        off = np.array([0.0, 0.0, 0.6])
        return (rng.normal(0, 0.05, (B, N, 3)) + off).astype(np.float32), (rng.normal(0, 0.05, (B, M, 3)) + off).astype(np.float32)
    return rng.normal(size=(B, N, C)).astype(np.float32), rng.normal(size=(B, M, C)).astype(np.float32)


# -------------------------------------------------------------------------------------------------- planted ball scenes
# Lattice coordinates are integers k, the point is k/64.  Query q sits at (CENTRE_X0 + CENTRE_DX q, 8, 8); the background fills
# y, z in [BG_LO, 64): at least BG_LO - 8 = 24 lattice steps from every centre, 16 steps beyond the widest ball (8 steps).
CENTRE_X0, CENTRE_YZ, BG_LO = 9, 8, 32


def ball_offsets(r2_steps, lo=1):
    """Integer offsets o with lo <= |o|^2 <= r2_steps, sorted by (|o|^2, o): the places hits are planted at, nearest first."""
    r = int(np.floor(np.sqrt(r2_steps)))
    g = np.arange(-r, r + 1)
    o = np.stack(np.meshgrid(g, g, g, indexing='ij'), -1).reshape(-1, 3)
    n2 = (o * o).sum(-1)
    o, n2 = o[(n2 >= lo) & (n2 <= r2_steps)], n2[(n2 >= lo) & (n2 <= r2_steps)]
    order = np.lexsort((o[:, 2], o[:, 1], o[:, 0], n2))
    return o[order]


def planted_scene(N, hits, r2_steps=9, centre_dx=10, place=None, shared=(), nan_at=(), seed=0):
    """-> dict(xyz (B,N,3), new_xyz (B,S,3) float64, hits).  hits[b][q]: the indices of cloud b that lie in the ball of query q (any
    order, disjoint between queries).  A ball is |o|^2 <= r2_steps lattice steps; the hits of a query take the offsets of
    ball_offsets(r2_steps) in list order (cyclically: a long list doubles points up), every other point is background.
    place[b]: {index: (q, offset)} puts single points at explicit offsets from centre q instead -- hits on the boundary or at the
    centre (list them in hits too), near misses outside (do not).  shared: pairs (q, q'): query q' sits where q does (give both
    the same hits).  nan_at[b]: indices whose x coordinate is NaN (members of every ball)."""
    B, S = len(hits), len(hits[0])
    rng = np.random.default_rng(seed)
    cq = np.array([[CENTRE_X0 + centre_dx * q, CENTRE_YZ, CENTRE_YZ] for q in range(S)])
    for q, q2 in shared:
        cq[q2] = cq[q]
    reach = int(np.ceil(np.sqrt(r2_steps)))
    assert cq[:, 0].max() + reach < 64 and CENTRE_YZ + reach + 8 <= BG_LO and (S < 2 or centre_dx >= 2 * reach + 4)
    offs = ball_offsets(r2_steps) if r2_steps >= 1 else np.zeros((1, 3), int)
    xyz = np.empty((B, N, 3))
    for b in range(B):
        k = np.concatenate([rng.integers(0, 64, (N, 1)), rng.integers(BG_LO, 64, (N, 2))], axis=1)
        fixed = dict(place[b]) if place else {}
        seen = set()
        for q in range(S):
            if any(q == q2 for _, q2 in shared):
                continue
            free = [i for i in hits[b][q] if i not in fixed]
            assert not seen & set(hits[b][q]) and all(0 <= i < N for i in hits[b][q]), 'hit lists overlap or leave the cloud'
            seen |= set(hits[b][q])
            for j, i in enumerate(free):
                k[i] = cq[q] + offs[j % len(offs)]
        for i, (q, o) in fixed.items():
            k[i] = cq[q] + np.asarray(o)
        assert k.min() >= 0 and k.max() < 64
        xyz[b] = k * STEP_XYZ
        for i in (nan_at[b] if nan_at else ()):
            xyz[b, i, 0] = np.nan
    new_xyz = np.broadcast_to(cq * STEP_XYZ, (B, S, 3)).copy()
    return dict(xyz=xyz, new_xyz=new_xyz, hits=hits, nan_at=nan_at)


def planted_rows(N, hits, nsample, nan_at=()):
    """The closed form of a planted scene: row (b, q) = sorted(H)[:ns] padded with min(H), H = hits[b][q] (and the NaN points, which
    every ball holds); N everywhere when H is empty.  ns = min(nsample, N)."""
    B, S = len(hits), len(hits[0])
    ns = min(int(nsample), N)
    out = np.full((B, S, ns), N, np.int64)
    for b in range(B):
        for q in range(S):
            H = sorted(set(hits[b][q]) | set(nan_at[b] if nan_at else ()))
            if H:
                out[b, q] = H[0]
                out[b, q, :min(ns, len(H))] = H[:ns]
    return out


# -------------------------------------------------------------------------------------------- general-value ball scenes
def ball_clearance(xyz, new_xyz, r2_f32):
    """(B,S) float64: min over the points of |sqdist_ref - r^2| - sqdist_bound, per query.  Positive: no float32 evaluation of the
    expansion within the bound can put any point of that row on the other side of r^2."""
    d = sqdist_ref(new_xyz, xyz)
    return (np.abs(d - np.float64(r2_f32)) - sqdist_bound(new_xyz, xyz)).min(axis=-1)


def general_ball_scene(B, N, S, r_nominal, seed, pool=None, tries=400):
    """-> dict(xyz (B,N,3), new_xyz (B,S,3) float32, radius (double), r2 (float32), clearance, candidate, queries (B,S)) or None.
    Clouds like test_primitives_gpu._cloud.  The candidates r2_j = float32(r_nominal^2 (1 + j 2^-12)), j = 0 .. tries - 1, are tried
    in order; the first one for which every query clears (ball_clearance > 0) is taken.  pool None: the queries are cloud points
    0 .. S - 1, so the condition covers every (query, point) pair.  pool = P > S: the queries are the first S of cloud points
    0 .. P - 1 that clear the candidate, for clouds so dense that no r^2 near the nominal one separates all pairs (with N = 2000,
    S = 100 a dozen pairs lie inside the bound of any r^2 near 0.03^2 -- 12 at the nominal one -- and none of the 400 candidates is
    free of them); the choice reads the reference and the bound only, and every row of the scene is then held to equality all the
    same.  `radius` is a double whose square rounds to r2 in float32: what query_ball_point is called with."""
    rng = np.random.default_rng(seed)
    xyz = (rng.normal(0, 0.05, (B, N, 3)) + np.array([0.0, 0.0, 0.6])).astype(np.float32)
    P = S if pool is None else pool
    cand = xyz[:, :P]
    d = sqdist_ref(cand, xyz)
    bound = sqdist_bound(cand, xyz)
    for j in range(tries):
        r2 = np.float32(r_nominal ** 2 * (1.0 + j * 2.0 ** -12))
        clear = (np.abs(d - np.float64(r2)) - bound).min(axis=-1)             # (B, P)
        ok = clear > 0
        if (ok.sum(axis=1) >= S).all():
            queries = np.stack([np.flatnonzero(ok[b])[:S] for b in range(B)])
            new_xyz = xyz[np.arange(B)[:, None], queries]
            radius = float(np.sqrt(np.float64(r2)))
            assert r2_of(radius) == r2
            return dict(xyz=xyz, new_xyz=new_xyz, radius=radius, r2=r2, candidate=j, queries=queries,
                        clearance=float(clear[np.arange(B)[:, None], queries].min()))
    return None


# --------------------------------------------------------------------------------------------------------- group scenes
def group_scene(B, N, S, K, D, seed):
    """-> dict(xyz (B,N,3), points (B,N,D) | None, new_xyz (B,S,3)) float32, general values.  Coordinates and centres are uniform in
    [0.25, 1): two binades, so the difference of two of them is a multiple of 2^-26 below 1 and exact in float64 -- float32 of the
    float64 difference IS the one correctly rounded float32 subtraction the kernel makes.  Rows 0 and N - 1 of the features hold
    PAYLOADS."""
    rng = np.random.default_rng(seed)
    xyz = rng.uniform(0.25, 1.0, (B, N, 3)).astype(np.float32)
    new_xyz = rng.uniform(0.25, 1.0, (B, S, 3)).astype(np.float32)
    points = with_payloads(rng.normal(size=(B, N, D)), (0, N - 1)) if D else None
    return dict(xyz=xyz, points=points, new_xyz=new_xyz)


def group_indices(kind, B, N, S, K, seed):
    """(B,S,K) int64: 'random' (uniform), 'same' (one index per cloud everywhere), 'last' (N - 1 everywhere)."""
    rng = np.random.default_rng(seed)
    if kind == 'random':
        return rng.integers(0, N, (B, S, K)).astype(np.int64)
    if kind == 'same':
        return np.broadcast_to(rng.integers(0, N, (B, 1, 1)), (B, S, K)).astype(np.int64)
    assert kind == 'last'
    return np.full((B, S, K), N - 1, np.int64)


# -------------------------------------------------------------------------------------------------------- bit patterns
PAYLOADS = np.array([0x80000000, 0x00000001, 0x807fffff, 0x7f800000, 0xff800000, 0x7fc00000, 0xffc12345, 0x7f800001, 0x7fffffff],
                    dtype=np.uint32).view(np.int32)     # -0.0, denormals, +-inf, quiet NaNs with payloads, a signalling NaN, all ones


def with_payloads(a, rows):
    """A copy of float32 array a (B,N,C) whose rows `rows` of every cloud hold PAYLOADS cyclically (shifted per cloud and row)."""
    a = np.array(a, np.float32)
    v = a.view(np.int32)
    for b in range(a.shape[0]):
        for j, r in enumerate(rows):
            v[b, r] = np.resize(np.roll(PAYLOADS, -(b + 2 * j)), a.shape[2])
    return a
