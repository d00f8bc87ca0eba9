"""The constructed traversal scenes (tests/collision_scenes.py) are what they claim, on the CPU: the C oracle returns the constructed codes,
nudges and pose bits and flips on the minus variant; float64 point-triangle distances certify the single witness and the margins; the
numpy restatement of the grid traversal (through MeshGrid._host_lists) gives the block visits, list lengths and queue fills a case is
named for.  A case that misses its own target fails here instead of passing silently on the device."""
import re

import numpy as np
import pytest

import collision_scenes as cs
from collision_scenes import RES
from oracle import collision_oracle as co

I4 = np.eye(4)
CASES = cs.cases()
IDS = [c.name for c in CASES]


def oracle(case):
    (V0, F0), (V1, F1) = case.mesh(0), case.mesh(1)
    return co.filter_grasp_pose(case.poses, case.syms, I4, I4, I4, I4, case.gig, 0, 0, case.adjust, V0, F0, V1, F1, case.points(0),
                                case.points(1), RES)


def same(got, exp, what):
    for g, x, name in zip(got, exp, ('codes', 'poses', 'nudge')):
        g = np.asarray(g); x = np.asarray(x)
        if name == 'poses':
            g = np.ascontiguousarray(g, dtype=np.float32).view(np.uint32); x = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
        assert np.array_equal(g, x), f'{what}: {name} differ: {g.tolist() if g.size < 40 else g.shape} vs {x.tolist() if x.size < 40 else ""}'


def geometric_hits(case):
    """The touching pairs of every tried pose, from float64 distances alone; asserts the margins on the way.
    -> ({e: {nudge index: side}}, {(e, idx): (side, key index, triangle index)})"""
    hits, pairs = {}, {}
    edge_margin = RES / 8.0 if case.group in ('E', 'G') else cs.MARGIN_CENTRE
    for e in range(case.E):
        for idx in cs.tries(case):
            found = []
            for side in (0, 1):
                keys = case.keys[side]
                if not len(keys):
                    continue
                T, _, _ = cs.posed_tris(case, side, e, idx)
                d, edge = cs.point_tri_dist((keys + 0.5) * RES, T)
                touch = d <= 0.1 * RES
                if case.corner is not None and case.corner[0] == side and (e, idx) == (case.wit[2], case.wit[3]):
                    v, t = case.corner[1], case.corner[2]
                    depth, second, clear = cs.corner_penetration((keys[v] + 0.5) * RES, T[t])
                    assert abs(depth - RES / 8.0) < 1e-3 * RES, depth / RES            # one corner, 1/8 voxel deep
                    assert second < -0.25 * RES and clear >= cs.MARGIN_CENTRE, (second / RES, clear / RES)
                    assert d[v, t] < cs.R_TOUCH
                    d[v, t] = np.inf
                    found.append((side, v, t))
                assert np.all(touch | (d >= cs.FAR)), f'{case.name}: a pair in the grey zone at e={e} idx={idx}: {d[~touch & (d < cs.FAR)] / RES}'
                for v, t in np.argwhere(touch):
                    assert edge[v, t] >= edge_margin - 1e-12, (case.name, edge[v, t] / RES)
                    if idx == 0:
                        assert d[v, t] < 1e-12, 'the centre of a lattice witness lies on its triangle'
                    found.append((side, int(v), int(t)))
            assert len(found) <= 1, f'{case.name}: {len(found)} touching pairs at e={e} idx={idx}'
            if found:
                hits.setdefault(e, {})[idx] = found[0][0]
                pairs[(e, idx)] = found[0]
    return hits, pairs


def declared(case):
    """the declared witnesses among the poses that the filter tries (without the nudge loop: the first only)"""
    d = {e: {i: s for i, s in h.items() if i in cs.tries(case)} for e, h in case.hits.items()}
    return {e: h for e, h in d.items() if h}


@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_case_is_what_it_claims(case):
    hits, pairs = geometric_hits(case)
    assert hits == declared(case), 'the declared witnesses are the touching pairs'
    exp = case.expected()
    same(oracle(case), exp, case.name)
    if case.wit is None:
        assert not any(case.hits.values())
        return
    side, vi, e, ti = case.wit
    assert pairs[(e, ti)][:2] == (side, vi)
    if case.group != 'F':                # lattice poses: the float32 cell lookup and the float64 restatement agree
        t = cs.traversal(case.variant(adjust=0, first_eval_only=True), side)
        assert t['border'] > 1e-5 and t['robust'], f'a voxel centre within {t["border"]} cells of a cell border'
    minus = case.variant(minus=True)
    mhits, _ = geometric_hits(minus)
    assert mhits == declared(minus)
    mexp = minus.expected()
    same(oracle(minus), mexp, case.name + ' minus')
    changed = (exp[0] != mexp[0]) | (exp[2] != mexp[2])
    assert changed[e] and changed.sum() == 1, 'exactly the witness evaluation flips'
    if not case.adjust:
        assert exp[0][e] == 3 + side and mexp[0][e] == 0 and mexp[2][e] == 0
    # keep_rejected_pose: a rejected evaluation keeps its composed pose
    kept = case.expected(keep_rejected_pose=True)
    assert np.array_equal(kept[1][exp[0] != 0], case.gic()[exp[0] != 0])


@pytest.mark.parametrize('case', [c for c in CASES if c.group == 'A'], ids=[c.name for c in CASES if c.group == 'A'])
def test_group_a_layout_and_mesh_voxels_collide(case):
    nf, wi, nk, where = re.match(r'A_nf(\d+)_w(\d+)_nk(\d+)_(first|last)', case.name).groups()
    nf, wi, nk = int(nf), int(wi), int(nk)
    _, pairs = geometric_hits(case)
    assert len(case.tris[0]) == nf and len(case.keys[0]) == nk
    assert pairs[(0, 0)] == (0, 0 if where == 'first' else nk - 1, wi)
    if 'degenerate' in case.name:
        T = case.tris[0]
        assert all(np.array_equal(T[j, 0], T[j, 1]) and np.array_equal(T[j, 0], T[j, 2]) for j in range(nf) if j != wi)
    if 'keymin' in case.name:
        assert case.keys[0][0].tolist() == [-32768, 32767, 0]
    V, F = case.mesh(0)
    # the witness triangle is the low corner of the mesh: its chunk's culling box ends at it
    assert np.all(case.tris[0][wi].min(axis=0) <= V.min(axis=0))
    gcam = case.gic()
    for keys, want in ((case.keys[0], [True, False]), (case.variant(minus=True).keys[0], [False, False])):
        assert [co.mesh_voxels_collide(V, F, gcam[e], keys, RES) for e in range(2)] == want


STATS = [c for c in CASES if c.stats]


@pytest.mark.parametrize('case', STATS, ids=[c.name for c in STATS])
def test_restated_traversal_is_the_one_the_case_is_named_for(case):
    side, vi = case.wit[0], case.wit[1]
    one = case.variant(adjust=0, first_eval_only=True)
    keys = one.keys[side]
    bx = one.boxes(side)
    for b in range(len(bx)):                                     # every box bounds its run of 64
        run = keys[b * 64:(b + 1) * 64]
        assert np.all(run >= bx[b, 0]) and np.all(run <= bx[b, 1])
    if case.group == 'F':
        s = np.diag(case.gig)[:3].astype(np.float32).astype(np.float64)
        assert (float((1.0 / s ** 2).sum()) <= 3.96) == (case.name == 'F_scale088')       # the grid's validity gate
        return
    tp = cs.traversal(one, side)
    tm = cs.traversal(one.variant(minus=True), side, g=tp['grid'])
    for t in (tp, tm):
        assert t['robust'], 'a block decision within the slack of its threshold'
        assert t['border'] > 1e-5, f'a voxel centre within {t["border"]} cells of a cell border'
    wb = vi // 64
    assert wb in tp['visited'], 'the witness block is visited'
    wt = len(case.tris[side]) - 1 if case.group == 'C' else 0
    assert (vi, wt) in tp['slot'], 'the witness pair is queued'
    A = RES / tp['grid']['cell']
    if case.group == 'B':
        m = re.match(r'B_last_q(\d+)', case.name)
        if m:
            assert vi == 64 * int(m.group(1)) == len(keys) - 1 and tp['visited'].tolist() == [wb]
        m = re.match(r'B_block(\d+)_lane(\d+)', case.name)
        if m:
            assert (wb, vi % 64) == (int(m.group(1)), int(m.group(2))) and len(keys) == 8192 and tp['visited'].tolist() == [wb]
            assert tm['visited'].tolist() == [wb] and tm['work0'] == (64 if wb < 127 else 63) and tm['work2'] == 1, 'the minus variant still visits the block'
        if case.name == 'B_beyond_table':
            assert len(keys) == 262144 + 65 and vi == len(keys) - 1 and wb == 4097 >= cs.BMASK_WORDS * 64
            assert tp['visited'].tolist() == [4096, 4097] and tp['work0'] == 65 and tm['work0'] == 64
    if case.group == 'C':
        assert tp['work2'] == case.pairs_total and tm['work2'] == case.pairs_total - case.wit_pairs
        assert len(tp['visited']) == tp['nblocks']
        last_flush = len(tp['flushes']) - 1
        if case.where != 'cap':
            assert tp['slot'][(vi, wt)] == ((0, 0) if case.where == 'first' else (last_flush, tp['flushes'][-1] - 1))
        if 'onepass' in case.name:
            assert tp['nblocks'] == 2 and tp['work2'] > 512 and tp['midpass'] and tm['midpass']
        if case.pairs_total == 1601:
            assert tm['work2'] > 1536 and len(tm['flushes']) >= 3
        if case.where == 'cap':
            assert tp['flushes'] == [cs.PAIR_CAP] and not tp['midpass'] and tp['nblocks'] == 2
        if case.pairs_total == 256:
            assert tp['flushes'][0] == cs.PAIR_DRAIN or case.where == 'last'
    if case.group == 'D':
        g = tp['grid']
        b = ((0.5 * RES - cs.posed_tris(one, side, 0, 0)[2]) - g['lo']) / g['cell']
        f0 = bx[:, 0] * A + b; f1 = bx[:, 1] * A + b
        assert tp['visited'].tolist() == [wb] and tp['work0'] == 64 < len(keys) and tm['visited'].tolist() == [wb] and tm['work0'] == 64
        if 'less_than_a_cell' in case.name:
            assert 0.0 < f1[wb, 0] < 1.0 and f0[wb, 0] < 0
            assert all(np.any(f1[k] < 0) for k in range(len(bx)) if k != wb)
        if 'straddles' in case.name:
            assert np.all(f0[wb] < 0) and np.all(f1[wb] >= g['dims']) and np.all((g['dims'] - 1) // 4 > 2)
        if 'empty_coarse' in case.name:
            assert np.all(f0[wb - 1] > 0) and np.all(f1[wb - 1] < g['dims'] - 1), 'the culled block lies inside the grid'
            assert cs.traversal(one, side, use_blocks=False, g=g)['work0'] == len(keys)


def test_group_e_covers_every_nudge_outcome():
    seen = set()
    for c in CASES:
        if c.group == 'E':
            co_, _, nu = c.expected()
            seen.add((c.adjust, int(co_[0]), int(nu[0])))
            assert co_[1] == 0 and nu[1] == 0
            T = c.tris[0][0]
            assert max(np.linalg.norm(T[i] - T[(i + 1) % 3]) for i in range(3)) <= 0.0004
    assert {(1, 0, n) for n in range(5)} | {(1, 3, -1), (0, 3, -1), (0, 4, -1), (0, 0, 0)} <= seen


def test_segment_table_rows():
    base, rows = cs.segment_table()
    assert len(rows) >= 40 and {n for _, n, _ in rows} == {0, 1, 2, 3} and {k for k, _, _ in rows} == {'wit', 'minus', 'novox'}
    codes, poses, nudge = cs.segment_expected(base, rows)
    assert len(codes) == sum(n for _, n, _ in rows) > 1024
    assert {(int(c), int(n)) for c, n in zip(codes, nudge)} == {(3, -1), (0, 1), (0, 0)}
    for kind in ('wit', 'minus'):
        for adjust in (0, 1):
            c = base.variant(minus=(kind == 'minus'), adjust=adjust, first_eval_only=True)
            same(oracle(c), c.expected(), f'segment row {kind} adjust={adjust}')
