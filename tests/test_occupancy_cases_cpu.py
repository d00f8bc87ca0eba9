"""The constructed rays, bitmaps and clouds of tests/occupancy_cases.py are what they claim, from the C oracle (oracle/collision_ref.c) alone:

  * `reference_ray` -- cast_ray over the leaf centres, then the float32 keep rule restated in occupancy_cases -- reproduces
    cr_make_occupancy_grid point for point on two small clouds, so it may stand for it;
  * every ray case has its constructed hit, end leaf and keep flag, at 2^-10 (where centres and queries are exact) and at 0.001f;
  * the tie cases depend on the tie rule (the oracle's `<=` variant decides them differently), the range cases on the order of the range
    and occupancy tests (the `range_last` variant), the keep-at-equality case on `<=` -- so each names a live branch;
  * the out-of-box rays do pass the cell next to the set bit: with that `ghost` cell occupied instead, the oracle reports a hit;
  * the wrapper clouds give non-empty reference results."""
import numpy as np
import pytest

import occupancy_cases as oc
from oracle import collision_oracle as co


def reference_ray(leaves, res, q, max_range):
    """-> hit, end (3,) float32, keep: one lattice point of cr_make_occupancy_grid"""
    pts = oc.centres(leaves, res) if len(leaves) else np.zeros((0, 3), dtype=np.float32)
    hit, end = co.cast_ray(pts, np.float32(res), oc.direction(q), np.float32(max_range))
    return hit, end, oc.keep_rule(q, hit, end)


def _outcome(ray, res, leaves=None):
    hit, end, keep = reference_ray(ray.leaves if leaves is None else leaves, res, ray.query(res), ray.range(res))
    key = tuple(int(v) for v in np.floor(end.astype(np.float64) / np.float64(res))) if hit else None
    return hit, key, keep


@pytest.mark.parametrize('name', ['axis-patch', 'integer-extent'])
def test_restated_keep_rule_is_the_oracle_grid(name):
    pts, res = oc.CLOUDS[name]()
    ref = co.make_occupancy_grid(pts, res)
    origin, n, max_range = oc.lattice_of(pts, res)
    lat = oc.lattice_points(origin, n, res)
    keep = np.zeros(len(lat), dtype=bool)
    for i, q in enumerate(lat):
        hit, end = co.cast_ray(pts, res, oc.direction(q), max_range)
        keep[i] = oc.keep_rule(q, hit, end)
    assert 0 < len(ref) < len(lat)
    assert np.array_equal(lat[keep].view(np.uint32), ref.view(np.uint32))


@pytest.mark.parametrize('res', [oc.RES, oc.RES_MM], ids=['2^-10', '0.001f'])
def test_ray_cases_have_their_constructed_outcome(res):
    cases = oc.ray_cases(res) + oc.border_cases()
    assert len({c.name for c in cases}) == len(cases)
    for ray in cases:
        assert all(abs(2 * v) == int(abs(2 * v)) for v in ray.q)
        if res == oc.RES:         # exact inputs
            assert np.array_equal(ray.query(res).astype(np.float64), np.array(ray.q) * 2.0 ** -10)
        hit, key, keep = _outcome(ray, res)
        assert (hit, key, keep) == (ray.hit, ray.end, ray.keep), f'{ray}: oracle {(hit, key, keep)}, constructed {(ray.hit, ray.end, ray.keep)}'


def test_issue_table_of_first_neighbours():
    t = {c.name: c for c in oc.tie_cases()}
    for sx in (1, -1):
        for sy in (1, -1):
            for sz in (1, -1):
                hits = [t[f'tie-octant{sx:+d}{sy:+d}{sz:+d}-axis{a}'].hit for a in range(3)]
                assert hits == ([False, False, True] if sz < 0 else [False, True, False] if sy < 0 else [True, False, False] if sx < 0
                                else [False, False, True])


def test_cases_sit_on_live_branches():
    try:
        co.set_occupancy_variant(tie=1)            # `<=`: x before y before z
        flipped = [r.name for r in oc.tie_cases() if _outcome(r, oc.RES)[0] != r.hit]
        assert {'tie-ppp-leaf(0, 0, 1)', 'tie-ppp-leaf(0, 1, 1)', 'tie-ppp-leaf(1, 0, 0)', 'tie-ppp-leaf(1, 1, 0)', 'tie-face(8, 8, 0)-first',
                'tie-face(8, 0, 8)-first', 'tie-face(0, 8, 8)-first'} <= set(flipped)
        assert any(n.startswith('tie-octant-1-1') for n in flipped)
        co.set_occupancy_variant(range_last=1)     # occupancy before range
        r = {c.name: c for c in oc.range_cases(oc.RES)}
        assert _outcome(r['range-20.5'], oc.RES)[0] and _outcome(r['range-float-below'], oc.RES)[0]
        co.set_occupancy_variant()
        lo, hi = oc.range_brackets(oc.RES)
        assert np.nextafter(lo, np.float32(1)) == hi
    finally:
        co.set_occupancy_variant()
    # keep at equality: dist == dist_query to the bit, so `<` would drop it
    q = oc.centres([(0, 0, 0)], oc.RES)[0]
    hit, end, keep = reference_ray([(0, 0, 0)], oc.RES, q, 0.0)
    assert hit and keep and np.array_equal(end, q)


def test_box_rays_pass_next_to_the_set_bit():
    for ray in oc.box_face_cases():
        for leaf in ray.leaves:                    # the set bits are inside the box, the ghost cell just outside it, next to one
            oc.bit_index(leaf, ray.offset)
        idx = [ray.ghost[a] - ray.offset[a] for a in range(3)]
        out = [a for a in range(3) if not 0 <= idx[a] < oc.DIMS[a]]
        assert len(out) == 1 and idx[out[0]] in (-1, oc.DIMS[out[0]])
        clamped = tuple(min(max(idx[a], 0), oc.DIMS[a] - 1) + ray.offset[a] for a in range(3))
        assert clamped in ray.leaves
        assert _outcome(ray, oc.RES) == (False, None, False)
        assert _outcome(ray, oc.RES, leaves=[ray.ghost])[:2] == (True, ray.ghost), ray
    faces = {(a, s) for ray in oc.box_face_cases() for a in range(3) for s in (-1, oc.DIMS[a]) if ray.ghost[a] - ray.offset[a] == s}
    assert len(faces) == 6


def test_bitmap_packing_and_lattice_inputs():
    assert oc.DIMS[0] * oc.DIMS[1] * oc.DIMS[2] == 105 and len(oc.pack([])) == 4
    for i in (0, 31, 32, 63, 64, 95, 96, 104):
        w = oc.pack([oc.key_of_bit(i)])
        assert oc.bit_index(oc.key_of_bit(i)) == i and w[i >> 5] == 1 << (i & 31) and np.count_nonzero(w) == 1
    assert sorted(oc.bit_index(k) for k in oc.corners()) == [0, 6, 28, 34, 70, 76, 98, 104]
    lat = oc.lattice_points(np.array(oc.LATTICE_ORIGIN, dtype=np.float32) * oc.RES, oc.LATTICE_N, oc.RES)
    assert len(lat) == 385 and len(lat) % 256 != 0
    i = (3 * 5 + 2) * 11 + 5
    assert not lat[i].any() and np.array_equal(lat[1], lat[0] + np.float32([0, 0, oc.RES]))       # q = 0 is on it; z fastest
    keep = [reference_ray(oc.LATTICE_LEAVES, oc.RES, q, oc.RANGE * float(oc.RES))[2] for q in lat]
    assert 20 < sum(keep) < 365


def test_wrapper_clouds_have_nonempty_references():
    for name, make in oc.CLOUDS.items():
        pts, res = make()
        assert len(pts) <= 200 and len(co.make_occupancy_grid(pts, res)) > 0, name
    pts, _ = oc.cloud_axis_patch()
    assert (pts[:, 0] == 0).any() and (pts[:, 1] == 0).any() and (pts[:, 0] < 0).any() and (pts[:, 1] > 0).any()
    pts, res = oc.cloud_origin_leaf()
    assert (co.voxelize(pts, res) == 0).all(axis=1).any()
    pts, res = oc.cloud_integer_extent()
    mx, mn = pts[:, 0].max(), pts[:, 0].min()
    ext = np.float32(np.float32(np.float32(mx + oc.PAD) - np.float32(mn - oc.PAD)) / res)
    assert ext == 26.0 and oc.lattice_of(pts, res)[1][0] == 26
