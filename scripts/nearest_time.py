"""dev: time of the unbounded nearest neighbour and the ball lists on the grid index (catgrasp_amd.neighbors) next to the brute-force
cg_nearest_neighbor -> profiles/nearest_time.json.

  python scripts/nearest_time.py          on the MI355X: HIP-event times, median of --reps after a warm-up

Frame, scene_pts and object: those of scripts/neighbors_time.py (synth.make_depth_image at 1544 x 2064 pixels; the 1 mm down-sampled
scene; the points within 3 cm of the frame's point nearest to the camera, thinned to several sizes).  The index is built as
neighbors.cKDTree builds it (default_cell).  Every row asserts equal indices before it times.
  (a) scene points within the gripper's radius of the object against the object (pipeline._background_points);
  (b) the whole scene against the object: most queries are far from it;
  (c) the object's 2 mm voxel centroids against the object (predicter.py:260);
  (d) ball_point of (a)'s queries at 0.005."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.join(HERE, '..')
sys.path.insert(0, ROOT)

OUT = os.path.join(ROOT, 'profiles', 'nearest_time.json')
K_REF = np.array([[2257.7500557850776, 0, 1032], [0, 2257.4882391629421, 772], [0, 0, 1]])
H_REF, W_REF = 1544, 2064


def main(reps, out_path, H, W, cell_scale=1.0):
    import torch
    from catgrasp_amd import _lib as L
    from catgrasp_amd import neighbors, scene, synth
    from catgrasp_amd._lib import _p, _stream
    from catgrasp_amd.aligning import voxel_down_sample_device
    dev = torch.device('cuda:0')
    K = K_REF.copy()
    K[0, 2], K[1, 2] = K[0, 2] * W / W_REF, K[1, 2] * H / H_REF
    lib = L.lib()

    def timed(fn):
        fn(); torch.cuda.synchronize()
        ms = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); out = fn(); b.record(); torch.cuda.synchronize()
            ms.append(a.elapsed_time(b))
        return round(statistics.median(ms), 4), out

    def brute(q, ref):
        idx = torch.empty((q.shape[0],), dtype=torch.int32, device=dev)
        ms, _ = timed(lambda: L.check(lib.cg_nearest_neighbor(_p(q), q.shape[0], _p(ref), ref.shape[0], _p(idx), _stream()), 'cg_nearest_neighbor'))
        return ms, idx

    def cell_of(ref):
        return cell_scale * neighbors.default_cell(ref.min(dim=0).values.tolist(), ref.max(dim=0).values.tolist(), ref.shape[0])

    def row_of(q, ref):
        """build + nearest of q against ref next to the brute-force pass; equal indices asserted first"""
        row = {'object_points': int(ref.shape[0]), 'queries': int(q.shape[0]), 'cell': cell_of(ref)}
        row['grid_build_ms'], index = timed(lambda: neighbors.GridIndex(ref, row['cell']))
        row['brute_force_nearest_ms'], want = brute(q, ref)
        idx, _, rounds = index.nearest(q, debug=True)
        assert torch.equal(idx, want), 'the grid and the brute-force pass disagree'
        row['nearest_ms'], _ = timed(lambda: index.nearest(q))
        row['queries_finished_by_the_linear_pass'] = int((rounds < 0).sum())
        row['mean_box_rounds'] = round(float(rounds.abs().double().mean()), 2)
        row['cells'] = index.ext
        return row, index

    depth = synth.make_depth_image(H, W, K, 60, seed=0)
    xyz, valid = scene.depth2xyzmap(depth, K, device=dev)
    P = xyz[valid].contiguous()
    scene_pts = voxel_down_sample_device(P.to(torch.float64), 0.001).contiguous()
    top = P[torch.argmin(P[:, 2])]
    obj = P[((P - top) ** 2).sum(dim=1) < 0.03 ** 2].to(torch.float64).contiguous()
    radius = synth.make_gripper()['diameter'] / 2
    _, nn = brute(scene_pts, obj)
    near = scene_pts[((scene_pts - obj[nn.long()]) ** 2).sum(dim=1) <= radius ** 2].contiguous()
    data = {'device': torch.cuda.get_device_name(0), 'reps': reps, 'image': [H, W], 'timer': 'HIP events, median', 'gripper_radius': radius,
            'cell_scale': cell_scale, 'scene_points': int(scene_pts.shape[0]), 'scene_points_within_the_gripper_radius': int(near.shape[0])}
    del xyz, valid, depth

    for name, q in (('a_scene_within_the_gripper_radius', near), ('b_whole_scene', scene_pts)):
        rows = []
        for size in (256, 1024, 4096, 16384, int(obj.shape[0])):
            if size > obj.shape[0]:
                continue
            ref = obj[torch.linspace(0, obj.shape[0] - 1, size, device=dev).long()].contiguous()
            rows.append(row_of(q, ref)[0])
            print(name, rows[-1], flush=True)
        data[name] = rows

    down = voxel_down_sample_device(obj, 0.002).contiguous()
    data['c_voxel_centroids_against_the_object'], index = row_of(down, obj)
    data['c_voxel_centroids_against_the_object']['voxel'] = 0.002
    print('c', data['c_voxel_centroids_against_the_object'], flush=True)

    d = {'object_points': int(obj.shape[0]), 'queries': int(near.shape[0]), 'radius': 0.005}
    d['grid_build_ms'], index = timed(lambda: neighbors.GridIndex(obj, 0.005))
    d['count_within_ms'], count = timed(lambda: index.count_within(near, 0.005))
    d['ball_point_ms'], (offsets, indices) = timed(lambda: index.ball_point(near, 0.005))
    assert torch.equal(torch.diff(offsets).to(torch.int32), count)
    d['indices'] = int(indices.shape[0])
    data['d_ball_point'] = d
    print('d', d, flush=True)

    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, 'w') as f:
        json.dump({'catgrasp_amd_on_mi355x': data}, f, indent=1, sort_keys=True)
        f.write('\n')


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out', default=OUT)
    ap.add_argument('--height', type=int, default=H_REF)
    ap.add_argument('--width', type=int, default=W_REF)
    ap.add_argument('--cell-scale', type=float, default=1.0, help='the index cell as a multiple of neighbors.default_cell (dev: to check the default)')
    args = ap.parse_args()
    main(args.reps, args.out, args.height, args.width, args.cell_scale)
