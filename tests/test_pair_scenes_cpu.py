"""The constructed inputs of tests/pair_scenes.py are what they claim, on the CPU.

  * every triangle verdict of the contact catalogue is decided by `exact_tri_tri`, an integer predicate written for this file: closed
    segment against closed triangle by the signs of integer determinants, in-plane cases by 2-D orientation signs.  It shares nothing
    with the kernel's separating axes or the oracle's clipping; the oracle must agree with it on every pair;
  * the restated axis expressions (pair_scenes.tri_axes / box_axes) prove the sole-separator claims, the box margins, that float32
    computes every lattice case without rounding, and that no filler pair collides;
  * the C oracle gives the constructed verdict on every scene and minus variant;
  * the launcher arithmetic, restated, shows that the scenes reach every thread, chunk and workgroup position they are named for.
A case that misses its own target fails here instead of passing silently on the device."""
import collections

import numpy as np

import pair_scenes as ps
from oracle import collision_oracle as co
from pair_scenes import RES


# ---------------------------------------------------------------------------------------------------------------------------------
# exact integer predicate (Python ints)
def _sub(a, b):
    return (a[0] - b[0], a[1] - b[1], a[2] - b[2])


def _crs(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def _dt(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def _sg(x):
    return (x > 0) - (x < 0)


def _o2(a, b, c):
    return _sg((b[0] - a[0]) * (c[1] - a[1]) - (b[1] - a[1]) * (c[0] - a[0]))


def _between(a, b, c):
    return min(a[0], b[0]) <= c[0] <= max(a[0], b[0]) and min(a[1], b[1]) <= c[1] <= max(a[1], b[1])


def _seg_seg2(a, b, c, d):
    o1, o2, o3, o4 = _o2(a, b, c), _o2(a, b, d), _o2(c, d, a), _o2(c, d, b)
    if o1 * o2 < 0 and o3 * o4 < 0:
        return True
    return ((o1 == 0 and _between(a, b, c)) or (o2 == 0 and _between(a, b, d)) or (o3 == 0 and _between(c, d, a))
            or (o4 == 0 and _between(c, d, b)))


def _in_tri2(x, v):
    s = [_o2(v[i], v[(i + 1) % 3], x) for i in range(3)]
    return not (1 in s and -1 in s)


def _seg_tri(a, b, v):
    """closed segment a-b (a == b: a point) against the closed proper triangle v"""
    n = _crs(_sub(v[1], v[0]), _sub(v[2], v[0]))
    assert any(n)
    da, db = _dt(n, _sub(a, v[0])), _dt(n, _sub(b, v[0]))
    if da * db > 0:
        return False
    ax = max(range(3), key=lambda i: abs(n[i]))
    u, w = (ax + 1) % 3, (ax + 2) % 3
    v2 = [(p[u], p[w]) for p in v]
    a2, b2 = (a[u], a[w]), (b[u], b[w])
    if da == 0 and db == 0:
        return _in_tri2(a2, v2) or _in_tri2(b2, v2) or any(_seg_seg2(a2, b2, v2[i], v2[(i + 1) % 3]) for i in range(3))
    if da == 0:
        return _in_tri2(a2, v2)
    if db == 0:
        return _in_tri2(b2, v2)
    s = [_sg(_dt(_crs(_sub(b, a), _sub(v[i], a)), _sub(v[(i + 1) % 3], a))) for i in range(3)]       # signed volumes (a, b, v_i, v_i+1)
    return not (1 in s and -1 in s)


def exact_tri_tri(P, Q):
    P = [tuple(int(x) for x in p) for p in np.asarray(P).reshape(3, 3)]
    Q = [tuple(int(x) for x in q) for q in np.asarray(Q).reshape(3, 3)]
    pz = not any(_crs(_sub(P[1], P[0]), _sub(P[2], P[0])))
    qz = not any(_crs(_sub(Q[1], Q[0]), _sub(Q[2], Q[0])))
    assert not (pz and qz)
    hit = False
    if not qz:
        hit |= any(_seg_tri(P[i], P[(i + 1) % 3], Q) for i in range(3))
    if not pz:
        hit |= any(_seg_tri(Q[i], Q[(i + 1) % 3], P) for i in range(3))
    return hit


def _runs(pairs):
    return [q for p in pairs for q in p.with_minus()]


def _f32_world(pair):
    """the pair as float32 world coordinates (what the kernel sees behind its pose chain)"""
    return ps.exact32(pair.A * RES), ps.exact32(pair.B * RES)


def _float32_is_exact(A_units, B_units):
    """tri_axes in float32 on the real coordinates and in int64 on the lattice units: the same masks and the same interval gaps"""
    A_units = np.asarray(A_units, dtype=np.int64).reshape(-1, 3, 3); B_units = np.asarray(B_units, dtype=np.int64).reshape(-1, 3, 3)
    s32, g32 = ps.tri_axes(ps.exact32(A_units * RES), ps.exact32(B_units * RES), dtype=np.float32)
    s64, g64 = ps.tri_axes(A_units, B_units, dtype=np.int64)
    deg = np.array([3] * 11 + [4] * 12, dtype=np.float64)              # an axis is a product of 2 (3) lengths, its projection one more
    return np.array_equal(s32, s64) and np.array_equal(g32.astype(np.float64), g64 * RES ** deg[None])


# ---------------------------------------------------------------------------------------------------------------------------------
# a. triangles
def test_triangle_catalogue_by_the_exact_predicate():
    runs = _runs(ps.tri_catalogue())
    count = collections.Counter()
    for p in runs:
        assert exact_tri_tri(p.A, p.B) == p.verdict, p.name
        a, b = _f32_world(p)
        assert co.tri_tri_overlap(a, b) == p.verdict, f'{p.name}: the oracle disagrees with the exact predicate'
        assert bool(ps.tri_hit(p.A[None], p.B[None], dtype=np.int64)[0]) == p.verdict, f'{p.name}: the restated axes (with the zero-area axes)'
        assert _float32_is_exact(p.A, p.B), p.name
        count[(p.cls, p.verdict)] += 1
    for p in ps.tri_catalogue():
        if p.minus is not None:
            d = np.abs(p.minus.A - p.A).sum() + np.abs(p.minus.B - p.B).sum()
            assert d == 3 or d == 3 * ps.FAR_STEP, 'the minus variant is one face moved by one lattice step (three vertices), or taken away'
    print('triangle catalogue (class, verdict): count', dict(sorted(count.items())))
    for cls in ('pierce', 'vertex-face', 'vertex-edge', 'vertex-vertex', 'edge-edge', 'collinear', 'coplanar', 'zero-area', 'zero-area-own-normal',
                'sole'):
        assert count[(cls, True)] >= 2 and count[(cls, False)] >= 2, cls
    assert count[('sole', True)] == count[('sole', False)] == 17 * 9 * 2


def test_touching_pairs_part_after_one_lattice_step():
    """every touching case (not the overlapping ones) has its minus variant exactly one lattice step away"""
    n = 0
    for p in ps.tri_contacts() + ps.tri_zero_area() + ps.tri_sole():
        if p.minus is None or p.minus.name.endswith('_away') or '_away_' in p.minus.name:
            continue
        moved = (p.minus.B - p.B) if np.any(p.minus.B != p.B) else (p.minus.A - p.A)
        assert np.all(moved == moved[0]) and np.abs(moved[0]).sum() == 1, p.name
        assert exact_tri_tri(p.A, p.B) and not exact_tri_tri(p.minus.A, p.minus.B)
        n += 1
    assert n >= 17 * 18 + 30
    print('touching pairs with a one-step minus variant:', n)


def test_zero_area_coplanar_miss_is_a_miss():
    """the closed segment passes the apex at a distance: only the segment's own in-plane normal separates.  Exact predicate and oracle
    say miss; the 17 axes alone say hit (the defect), with the zero-area axes the restatement says miss."""
    n = 0
    for p in _runs(ps.tri_zero_area()):
        if p.cls != 'zero-area-own-normal' or p.verdict:
            continue
        assert not exact_tri_tri(p.A, p.B)
        a, b = _f32_world(p)
        assert not co.tri_tri_overlap(a, b)
        assert bool(ps.tri_hit(a[None], b[None], zero_area_axes=False)[0]), 'none of the 17 axes separates this pair'
        sep, _ = ps.tri_axes(a[None], b[None])
        assert sep[0, 17:].any() and not sep[0, :17].any()
        n += 1
    assert n == 4                                          # two vertex orders, both argument orders


def test_each_of_the_17_axes_is_the_sole_separator():
    decided = collections.Counter()
    for p in ps.tri_sole():
        k = ps.sole_axis(p.minus)                          # asserts: exactly one axis separates
        sep, gap = ps.tri_axes(p.A[None], p.B[None], dtype=np.int64)
        assert not sep.any() and gap[0, k] == 0, f'{p.name}: the twin touches with gap 0 on axis {k}'
        order = 'ba' if '_ba' in p.name else 'ab'
        decided[(order, k)] += 1
    for order in ('ab', 'ba'):
        assert sorted(k for o, k in decided if o == order) == list(range(17)), 'every axis decides in both argument orders'
    print('sole-separator variants per (argument order, axis):', dict(sorted(decided.items())))
    assert sum(decided.values()) == 17 * 18


# ---------------------------------------------------------------------------------------------------------------------------------
# b. cubes
def _cube_e(p, dtype=np.float64):
    t = ps.cloud_t(p.ka[None], ps.RES_A, p.kb[None], p.res_b, p.rel, dtype=dtype)[0]
    return t[0], ps.box_axes(t, 0.5 * ps.RES_A, 0.5 * p.res_b, p.rel[:3, :3], dtype=dtype)[0]


def test_cube_catalogue():
    count = collections.Counter()
    sole = collections.Counter()
    assert ps.ROT_MARGIN >= 64 * ps.ROT_BOUND
    for p in _runs(ps.cube_catalogue()):
        h = 0.5 * (ps.RES_A + p.res_b)
        t, e = _cube_e(p)
        inside = bool(np.all(np.abs(t) < 0.99 * float(ps.reach_of(ps.RES_A, p.res_b))))
        assert inside or p.name.endswith('_away'), f'{p.name}: the pair passes the reach reject'
        assert bool(np.all(e <= 0)) == p.verdict, p.name
        ca = ps.centres(p.ka, ps.RES_A)[0]
        assert co.box_box_overlap(ca, 0.5 * ps.RES_A, ca + t, 0.5 * p.res_b, p.rel[:3, :3]) == p.verdict, f'{p.name}: the oracle'
        if p.exact:
            t32, e32 = _cube_e(p, np.float32)
            assert np.array_equal(t32.astype(np.float64), t) and np.array_equal(e32.astype(np.float64), e), f'{p.name}: float32 is exact'
            assert np.all(np.abs(p.rel[:3, :3]).sum(axis=0) == 1) and np.all(np.abs(p.rel[:3, :3]).sum(axis=1) == 1)
            if not p.verdict and p.name.endswith('_apart'):
                assert np.isclose(e.max(), 0.5 * ps.RES_A, rtol=0, atol=0), 'half a step of the finer resolution apart'
        else:
            assert np.all(np.abs(e) >= ps.ROT_MARGIN * h), f'{p.name}: margin {np.abs(e).min() / h}'
            assert [int(k) for k in np.nonzero(e > 0)[0]] == ([] if p.verdict else [p.sole])
            sole[(p.sole, p.verdict)] += 1
        count[(p.cls, 'eq' if p.res_b == ps.RES_A else '2:1', p.verdict)] += 1
        if 'int16' in p.cls:
            assert set(np.abs(np.concatenate([p.ka, p.kb]) + 0.5)) == {32767.5}
    print('cube catalogue (class, resolutions, verdict): count', dict(sorted(count.items())))
    assert sorted(sole) == [(k, v) for k in range(15) for v in (False, True)]
    for cls in ('aligned', 'aligned_int16'):
        for r in ('eq', '2:1'):
            assert count[(cls, r, True)] and count[(cls, r, False)]
    kinds = {p.name.split('_')[0] for p in ps.cube_aligned()}
    assert kinds == {'face', 'edge', 'corner', 'identical', 'inside'}


# ---------------------------------------------------------------------------------------------------------------------------------
# c. scenes
def _units(x):
    u = np.asarray(x, dtype=np.float64) / RES
    assert np.array_equal(u, np.round(u))
    return u.astype(np.int64)


def _mesh_proof(s):
    """-> (hits [(ia, ib)], partnered fillers, fillers): every pair whose boxes overlap goes through the restated predicate"""
    ta, tb = _units(s.world(0)), _units(s.world(1))
    la, ha_, lb, hb_ = ta.min(1), ta.max(1), tb.min(1), tb.max(1)
    ia, ib = s.at
    if s.capped:                                             # the fillers as two blocks, the pair against everything
        fa, fb = np.delete(np.arange(len(ta)), ia), np.delete(np.arange(len(tb)), ib)
        assert np.any(la[fa].min(0) > hb_[fb].max(0)) or np.any(ha_[fa].max(0) < lb[fb].min(0)), 'filler blocks apart'
        pa = np.nonzero(np.all((la[ia][None] <= hb_) & (ha_[ia][None] >= lb), axis=1))[0]
        pb = np.nonzero(np.all((la <= hb_[ib][None]) & (ha_ >= lb[ib][None]), axis=1))[0]
        cand = sorted({(ia, int(j)) for j in pa} | {(int(i), ib) for i in pb})
    else:
        ov = np.all((la[:, None, :] <= hb_[None, :, :]) & (ha_[:, None, :] >= lb[None, :, :]), axis=2)
        cand = [(int(i), int(j)) for i, j in np.argwhere(ov)]
    if not cand:
        return [], 0, len(ta) + len(tb) - 2
    A = np.stack([ta[i] for i, _ in cand]); B = np.stack([tb[j] for _, j in cand])
    assert np.abs(B - A[:, :1]).max() <= 24, 'pairs that pass the box reject are small: every product stays below 2**24'
    assert _float32_is_exact(A, B)
    hit = ps.tri_hit(A, B, dtype=np.int64)
    hits = [c for c, h in zip(cand, hit) if h]
    fill = [c for c in cand if c[0] != ia and c[1] != ib]
    partnered = len({i for i, _ in fill}) + len({j for _, j in fill})
    return hits, partnered, len(ta) + len(tb) - 2


def _check_mesh_scene(s, stats):
    assert not np.array_equal(s.pose_a, np.eye(4)) and not np.array_equal(s.pose_b, np.eye(4))
    for V, F, w in ((s.VA, s.FA, s.at[0]), (s.VB, s.FB, s.at[1])):
        used = np.zeros(len(V), dtype=bool); used[F.reshape(-1)] = True
        assert np.all(np.isnan(V[~used])) and not np.any(np.isnan(V[used])) and (~used).sum() >= 1
        assert sorted(F[w].tolist()) == [len(V) - 3, len(V) - 2, len(V) - 1], 'the witness uses the highest vertex indices'
    hits, partnered, fillers = _mesh_proof(s)
    assert hits == ([s.wit] if s.verdict else []), (s.name, hits[:5])
    stats['fillers'] += fillers; stats['partnered'] += partnered
    return partnered, fillers


def test_mesh_scenes_have_one_witness_and_the_oracle_agrees():
    stats = collections.Counter()
    scenes = ps.mesh_traversal_scenes() + ps.mesh_catalogue_scenes() + ps.mesh_catalogue_scenes(embedded=True)
    for s0 in scenes:
        assert s0.verdict == (s0.wit is not None)
        for s in s0.with_minus():
            partnered, fillers = _check_mesh_scene(s, stats)
            if min(s.shape) >= 64:
                assert 4 * partnered >= fillers, f'{s.name}: {partnered} of {fillers} fillers have a box that overlaps a filler of the other set'
            assert co.mesh_mesh_collide(s.VA, s.FA, s.pose_a, s.VB, s.FB, s.pose_b) == s.verdict, s.name
            stats['scenes'] += 1
        assert s0.minus is None or not s0.minus.verdict
    print(f'mesh scenes: {stats["scenes"]}; fillers {stats["fillers"]}, of which {stats["partnered"]} overlap a box of the other set')
    assert 4 * stats['partnered'] >= stats['fillers']
    s = ps.mesh_self_scene()
    assert s.verdict and co.mesh_mesh_collide(s.VA, s.FA, s.pose_a, s.VB, s.FB, s.pose_b)
    assert ps.launch(*s.shape)[:2] == (5, 5)


def test_mesh_capped_scenes():
    stats = collections.Counter()
    """the vectorised box proof covers all six capped shapes; the oracle (1.5 s for a full scan of 2.5e8 pairs) runs on the first and the last"""
    for i, s0 in enumerate(ps.mesh_capped_scenes()):
        for s in s0.with_minus():
            assert s.capped
            _check_mesh_scene(s, stats)
            if i in (0, 5):
                assert co.mesh_mesh_collide(s.VA, s.FA, s.pose_a, s.VB, s.FB, s.pose_b) == s.verdict, s.name


def _cloud_proof(s):
    """every pair of cubes: beyond reach by a clear factor, or separated by a clear margin, or the witness"""
    h = 0.5 * (s.res_a + s.res_b)
    reach = float(ps.reach_of(s.res_a, s.res_b))
    ia, ib = s.at
    if s.capped:
        fa, fb = np.delete(s.keys_a, ia, axis=0), np.delete(s.keys_b, ib, axis=0)
        r = s.rel.astype(np.float64)
        cb = ps.centres(fb, s.res_b) @ r[:3, :3].T + r[:3, 3]
        ca = ps.centres(fa, s.res_a)
        assert np.any(cb.min(0) - ca.max(0) > 2 * reach) or np.any(ca.min(0) - cb.max(0) > 2 * reach), 'filler blocks beyond reach'
        t1 = ps.cloud_t(s.keys_a[ia:ia + 1], s.res_a, s.keys_b, s.res_b, s.rel)[0]
        t2 = ps.cloud_t(s.keys_a, s.res_a, s.keys_b[ib:ib + 1], s.res_b, s.rel)[:, 0]
        t = np.concatenate([t1, t2]); idx = [(ia, j) for j in range(len(t1))] + [(i, ib) for i in range(len(t2))]
    else:
        t = ps.cloud_t(s.keys_a, s.res_a, s.keys_b, s.res_b, s.rel).reshape(-1, 3)
        idx = None
    near = np.nonzero(np.all(np.abs(t) <= 1.01 * reach, axis=1))[0]
    e = ps.box_axes(t[near], 0.5 * s.res_a, 0.5 * s.res_b, s.rel[:3, :3], dtype=np.float64)
    hits, partner_a, partner_b = [], set(), set()
    for n, row in zip(near, e):
        i, j = idx[n] if idx is not None else divmod(int(n), len(s.keys_b))
        if (i, j) == (ia, ib):
            if np.all(row <= 0):
                hits.append((i, j))
            continue
        assert row.max() >= 8 * ps.ROT_MARGIN * h, f'{s.name}: filler pair {(i, j)} is not clearly separated ({row.max() / h})'
        if np.all(np.abs(t[n]) <= 0.99 * reach) and i != ia and j != ib:
            partner_a.add(i); partner_b.add(j)
    return sorted(set(hits)), len(partner_a) + len(partner_b), len(s.keys_a) + len(s.keys_b) - 2


def _oracle_cloud(s):
    return co.voxels_voxels_collide(s.keys_a, s.res_a, s.keys_b, s.res_b, s.rel)


def test_cloud_scenes_have_one_witness_and_the_oracle_agrees():
    stats = collections.Counter()
    scenes = ps.cloud_traversal_scenes() + ps.cloud_catalogue_scenes() + ps.cloud_catalogue_scenes(embedded=True) + ps.cloud_capped_scenes()
    for s0 in scenes:
        for s in s0.with_minus():
            hits, partnered, fillers = _cloud_proof(s)
            assert hits == ([s.wit] if s.verdict else []), (s.name, hits[:5])
            assert _oracle_cloud(s) == s.verdict, s.name
            if not s.capped:
                stats['fillers'] += fillers; stats['partnered'] += partnered
            if s.cls == 'traversal' and min(s.shape) >= 64:
                assert 4 * partnered >= fillers, (s.name, partnered, fillers)
            stats['scenes'] += 1
    # aligned cubes of EQUAL size sit on one lattice: a cube inside `reach` of another touches it, so those embedded scenes have no
    # partnered fillers; the quarter holds over all scenes and in every traversal scene
    print(f'cloud scenes: {stats["scenes"]}; fillers {stats["fillers"]}, of which {stats["partnered"]} pass the reach reject against a filler')
    assert 4 * stats['partnered'] >= stats['fillers']
    s = ps.cloud_self_scene()
    assert _oracle_cloud(s) and ps.launch(*s.shape)[:2] == (5, 5)


# ---------------------------------------------------------------------------------------------------------------------------------
# reach: the launcher's arithmetic
def test_scenes_reach_every_position():
    pos = ps.traversal_positions()
    w = [ps.where(p[0], p[2], p[1], p[3]) for p in pos]
    seen_a = {(na, ia) for na, ia, _, _ in pos}
    for na in (1, 255, 256, 257, 513):
        for ia in (0, 63, 64, 255, 256, na - 1):
            if ia < na:
                assert (na, ia) in seen_a, (na, ia)
    seen_b = {(nb, ib) for _, _, nb, ib in pos}
    assert {nb % 256 for nb, _ in seen_b} == {0, 1, 255} and {(nb + 255) // 256 for nb, _ in seen_b} == {2, 3}
    for nb in {nb for nb, _ in seen_b}:
        assert {(nb, ib) for ib in (0, 255, 256, nb - 1)} <= seen_b
    assert {d['thread'] for d in w} >= {0, 63, 64, 255, 254} and {d['x'] for d in w} == {0, 1, 2}
    assert {d['y'] for d in w} == {0, 1, 2} and {d['lane'] for d in w} >= {0, 255, 254} and all(d['per'] == 1 for d in w)
    assert any(d['last_chunk'] and d['lane'] == 0 for d in w), 'a last chunk of one element'
    for s, p in zip(ps.mesh_traversal_scenes(), pos):
        assert s.shape == (p[0], p[2]) and s.at == (p[1], p[3]) and s.minus.shape == s.shape
    for s, p in zip(ps.cloud_traversal_scenes(), pos):
        assert s.shape == (p[0], p[2]) and s.at == (p[1], p[3]) and s.minus.shape == s.shape
    # the capped grid
    cw = [ps.where(p[0], p[2], p[1], p[3]) for p in ps.capped_positions()]
    d = cw[0]
    assert d['gx'] * d['chunks'] > ps.CAP and d['per'] == 2 and d['gx'] * d['gy'] <= ps.CAP and d['chunks_of_last_y'] == 1 < d['per']
    assert {(c['slot'], c['last_chunk']) for c in cw} == {(0, False), (1, False), (0, True)}
    assert {c['x'] for c in cw} == {0, d['gx'] - 1} and d['gx'] == 17 and d['gy'] == 122
    print(f'capped shape {ps.CAPPED_NA} x {ps.CAPPED_NB}: gx {d["gx"]}, gy {d["gy"]}, per {d["per"]}, chunks {d["chunks"]}; witnesses at',
          [(c['x'], c['thread'], c['y'], c['slot'], c['lane']) for c in cw])
    e = ps.where(*ps.EMBED)
    assert e['thread'] not in (0, 255) and e['chunk'] == 1 and e['lane'] not in (0, 255)
    for s in ps.mesh_capped_scenes() + ps.cloud_capped_scenes():
        assert s.capped and s.shape == (ps.CAPPED_NA, ps.CAPPED_NB) and s.minus.shape == s.shape
    print('traversal positions (na, ia, nb, ib):', pos)
