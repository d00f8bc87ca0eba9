"""Golden vectors for pointgroup_ops.bfs_cluster on neighbour lists that the ball query's 1000-neighbour cap has cut, from the
REFERENCE'S OWN C++ queue BFS (bfs_cluster.cpp:33-91, compiled by oracle/build_ref.py:build_pointgroup_host into
oracle/_ref/libpointgroup_host_ref.so).  Build container only.

The reference runs ballquery_batch_p on offset-shifted coordinates, where an object's points collapse onto its centre: more than
1000 in-radius neighbours per point is the normal case there.  A cut list keeps the first 1000 in-radius indices in ascending
order, so a high-index point of a tight blob lists the blob's first 1000 points and nobody lists it: the relation is one-way, and the
queue BFS, which follows lists one way, leaves such points out of the blob's cluster.

Scenes (radius 0.03, random index order):
  blob1300  blobs of 1300 and 400 points (sigma 0.002) + 30 far points, one label
  bridged   blobs of 1200, 300 and 200 points at x = 0, 0.026, 0.052 + 20 far points, two labels interleaved
  bar       1500 points along a 0.08 bar + a far blob of 180 + 20 far points, two labels on the blob: lists are cut, yet every point
            is still listed by a neighbour, and the one-way clusters equal the undirected components
Stored per scene: xyz, label, the per-point neighbour counts and the reference's cluster_idxs / cluster_offsets at thresholds 1 and
50.  The neighbour array itself (about 1.5 M entries per scene) is not stored: tests rebuild it from xyz.

    python tests/golden/make_golden_pointgroup_cap.py   ->   tests/golden/pointgroup_cap_golden.npz
"""
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle import build_ref  # noqa: E402
from oracle import pointgroup_ops_ref as ref  # noqa: E402

RADIUS = 0.03
CAP = 1000
THRESHOLDS = (1, 50)


def scenes():
    """name -> (xyz float32, label int32), seeded."""
    rng = np.random.default_rng(1300)
    far = lambda m: rng.uniform(5, 9, (m, 3))
    blob = lambda c, m: rng.normal(c, 0.002, (m, 3))
    out = {}
    xyz = np.concatenate([blob((0, 0, 0), 1300), blob((0.5, 0, 0), 400), far(30)])
    out['blob1300'] = (xyz, np.zeros(len(xyz), dtype=np.int32))
    xyz = np.concatenate([blob((0, 0, 0), 1200), blob((0.026, 0, 0), 300), blob((0.052, 0, 0), 200), far(20)])
    out['bridged'] = (xyz, rng.integers(0, 2, len(xyz)).astype(np.int32))
    bar = np.stack([rng.uniform(0, 0.08, 1500), rng.normal(0, 0.001, 1500), rng.normal(0, 0.001, 1500)], 1)
    xyz = np.concatenate([bar, blob((0.5, 0.5, 0), 180), far(20)])
    label = np.zeros(len(xyz), dtype=np.int32); label[1500:1680] = rng.integers(0, 2, 180)
    out['bar'] = (xyz, label)
    for name, (xyz, label) in out.items():
        perm = rng.permutation(len(xyz))
        out[name] = (np.ascontiguousarray(xyz[perm], dtype=np.float32), np.ascontiguousarray(label[perm]))
    return out


def undirected_components(label, idx, start_len):
    """comp[v] = smallest index of v's connected component when every list entry is read as an undirected same-label edge."""
    src = np.repeat(np.arange(len(start_len)), start_len[:, 1]); dst = idx.astype(np.int64)
    same = label[src] == label[dst]
    src, dst = src[same], dst[same]
    comp = np.arange(len(start_len))
    while True:
        new = comp.copy()
        np.minimum.at(new, dst, comp[src]); np.minimum.at(new, src, comp[dst])
        new = np.minimum(new, new[new])
        if np.array_equal(new, comp):
            return comp
        comp = new


def main():
    lib = ctypes.CDLL(build_ref.build_pointgroup_host())
    fp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    out = {'radius': np.float32(RADIUS), 'scenes': np.array(sorted(scenes()))}
    for name, (xyz, label) in scenes().items():
        n = len(xyz)
        idx, start_len, _ = ref.ballquery_batch_p(xyz, np.zeros(n, dtype=np.int32), np.array([0, n], dtype=np.int32), RADIUS, 300)
        idx = np.ascontiguousarray(idx, dtype=np.int32); start_len = np.ascontiguousarray(start_len, dtype=np.int32)
        counts = start_len[:, 1].copy()
        assert counts.max() == CAP and (counts == CAP).sum() > 0, f'{name}: no capped point'
        out[f'{name}_xyz'] = xyz; out[f'{name}_label'] = label; out[f'{name}_counts'] = counts
        und = undirected_components(label, idx, start_len)
        for thr in THRESHOLDS:
            s = ctypes.c_int(0)
            nc = lib.ref_bfs_cluster(fp(label), fp(idx), fp(start_len), n, thr, ctypes.byref(s), None, None)
            ci = np.zeros((s.value, 2), dtype=np.int32); co = np.zeros((nc + 1,), dtype=np.int32)
            lib.ref_bfs_cluster(fp(label), fp(idx), fp(start_len), n, thr, ctypes.byref(s), fp(ci), fp(co))
            out[f'{name}_thr{thr}_cluster_idxs'] = ci; out[f'{name}_thr{thr}_cluster_offsets'] = co
        # threshold 1 keeps every point: owner[v] = first (= smallest, the seed) member of v's cluster
        ci, co = out[f'{name}_thr1_cluster_idxs'], out[f'{name}_thr1_cluster_offsets']
        assert len(ci) == n
        owner = np.zeros(n, dtype=np.int64); owner[ci[:, 1]] = ci[co[:-1], 1][ci[:, 0]]
        differs = not np.array_equal(owner, und)
        assert differs == (name != 'bar'), f'{name}: one-way clusters {"differ from" if differs else "equal"} the undirected components'
        sizes50 = np.diff(out[f'{name}_thr50_cluster_offsets'])
        assert len(sizes50) >= 2, f'{name}: fewer than two clusters at threshold 50'
        print(f'{name}: n {n}, capped {int((counts == CAP).sum())}, entries {len(idx)}, reference clusters {len(co) - 1} '
              f'(threshold 50: {sizes50.tolist()}), undirected components {len(np.unique(und))} '
              f'(>= 50: {sorted(np.bincount(und)[np.bincount(und) >= 50].tolist(), reverse=True)})')
    path = os.path.join(ROOT, 'tests', 'golden', 'pointgroup_cap_golden.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
