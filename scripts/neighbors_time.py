"""dev: time of the grid index (catgrasp_amd.neighbors) at the reference camera -> profiles/neighbors_time.json.

  python scripts/neighbors_time.py          on the MI355X: HIP-event times, median of --reps after a warm-up

Frame: the one of scripts/scene_time.py (synth.make_depth_image at 1544 x 2064 pixels, a floor plane at about 0.65 m and 60 spheres, no
background mask).  Build (GridIndex(...): finiteness check, bounding box, key kernel, stable sort, gathers -- it synchronises twice) and
query are timed apart:
  (a) the normals of xyz_map[use] at radius 0.002 through the grid, next to cg_organized_normals on the same frame in the same run
      (both give the same bits there, which is checked);
  (b) the normals of the 1 mm scene_pts at radius 0.003 (run_grasp_simulation.py:247-248);
  (c) nearest_within and count_within of scene_pts against the points of one object at radius 0.005, next to the brute-force
      cg_nearest_neighbor on the same inputs, for the object thinned to several sizes (the brute force is one pass over all of them per
      query; the grid pays a build and a sort of the queries)."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.join(HERE, '..')
sys.path.insert(0, ROOT)

OUT = os.path.join(ROOT, 'profiles', 'neighbors_time.json')
K_REF = np.array([[2257.7500557850776, 0, 1032], [0, 2257.4882391629421, 772], [0, 0, 1]])
H_REF, W_REF = 1544, 2064


def main(reps, out_path, H, W):
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

    depth = synth.make_depth_image(H, W, K, 60, seed=0)
    xyz, valid = scene.depth2xyzmap(depth, K, device=dev)
    data = {'device': torch.cuda.get_device_name(0), 'reps': reps, 'image': [H, W], 'max_nn': 30, 'timer': 'HIP events, median'}

    # (a) the organized cloud both ways
    P = xyz[valid].contiguous()
    a = {'points': int(P.shape[0]), 'radius': 0.002}
    hu, hv = scene.window_halfwidths(xyz, valid, K, 0.002)
    use_u8 = valid.to(torch.uint8).contiguous()
    organized = torch.empty((H, W, 3), dtype=torch.float64, device=dev)

    def organized_kernel():                                  # the bare kernel on ready buffers, as scripts/scene_time.py times it
        L.check(lib.cg_organized_normals(_p(xyz), _p(use_u8), H, W, K[0, 0], K[1, 1], K[0, 2], K[1, 2], 0.002, 30, 0.0, 0.0, 0.0, 0, hu, hv,
                                         _p(organized), None, None, _stream()), 'cg_organized_normals')
    a['organized_normals_ms'], _ = timed(organized_kernel)
    a['grid_build_ms'], index = timed(lambda: neighbors.GridIndex(P, 0.002))
    a['grid_normals_ms'], normals = timed(lambda: index.estimate_normals(0.002, 30))
    a['same_bits_as_organized'] = bool(torch.equal(normals, organized[valid]))
    a['cells'] = index.ext
    data['a_frame_cloud'] = a
    print(a, flush=True)
    del organized, normals, index

    # (b) the down-sampled scene
    scene_pts = voxel_down_sample_device(P.to(torch.float64), 0.001).contiguous()
    b = {'points': int(scene_pts.shape[0]), 'radius': 0.003}
    b['grid_build_ms'], index = timed(lambda: neighbors.GridIndex(scene_pts, 0.003))
    b['grid_normals_ms'], normals = timed(lambda: index.estimate_normals(0.003, 30, debug=True))
    b['mean_neighbours'] = round(float(normals[1].double().mean()), 2)
    b['cells'] = index.ext
    data['b_scene_pts'] = b
    print(b, flush=True)
    del normals, index

    # (c) radius queries of scene_pts against one object: the points within 3 cm of the frame's point nearest to the camera
    top = P[torch.argmin(P[:, 2])]
    obj = P[((P - top) ** 2).sum(dim=1) < 0.03 ** 2].to(torch.float64).contiguous()
    rows = []
    idx = torch.empty((scene_pts.shape[0],), dtype=torch.int32, device=dev)
    for size in (256, 1024, 4096, 16384, int(obj.shape[0])):
        if size > obj.shape[0]:
            continue
        ref = obj[torch.linspace(0, obj.shape[0] - 1, size, device=dev).long()].contiguous()
        row = {'object_points': size, 'queries': int(scene_pts.shape[0]), 'radius': 0.005}
        row['grid_build_ms'], index = timed(lambda: neighbors.GridIndex(ref, 0.005))
        row['nearest_within_ms'], near = timed(lambda: index.nearest_within(scene_pts, 0.005))
        row['count_within_ms'], cnt = timed(lambda: index.count_within(scene_pts, 0.005))
        row['brute_force_nearest_ms'], _ = timed(lambda: L.check(lib.cg_nearest_neighbor(_p(scene_pts), scene_pts.shape[0], _p(ref), size, _p(idx),
                                                                                         _stream()), 'cg_nearest_neighbor'))
        found = near[0] >= 0
        d2 = ((scene_pts - ref[idx.long()]) ** 2).sum(dim=1)
        row['queries_with_a_point_in_range'] = int(found.sum())
        row['agrees_with_brute_force'] = bool(torch.equal(found, cnt > 0) and torch.equal(near[0][found], idx[found]) and bool((d2[~found] > 0.005 ** 2).all()))
        rows.append(row)
        print(row, flush=True)
    data['c_scene_pts_against_one_object'] = rows
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
    args = ap.parse_args()
    main(args.reps, args.out, args.height, args.width)
