"""dev: time of the scene front end (catgrasp_amd.scene) at the reference camera -> profiles/scene_time.json.

  python scripts/scene_time.py          on the MI355X: HIP-event times, median of --reps after a warm-up

Frame: synth.make_depth_image at the reference's camera (config.yml: 1544 x 2064 pixels, K below), a floor plane at about 0.65 m and 60
spheres; no background mask, so every pixel is used.

Timed:
  cg_depth_to_xyz and cg_organized_normals alone, on ready device buffers (the normals on both routes, and which one AUTO takes);
  the whole scene.scene_from_depth call from a depth image in host memory (upload, both kernels, the half-width reduction, compaction,
  voxel down-sampling, all left on the device).
Counted from the shapes: used points, and candidate evaluations = the window sizes of all used pixels (one scan of every window; a
query with more than max_nn points in range scans its window several more times, which is not counted).
Beside them, informational: the same normals on the host for a crop of about 100,000 points -- scipy's cKDTree hybrid query
(k = 30 within the radius) + a batched numpy eigh, the work open3d does on the host in the reference."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.join(HERE, '..')
sys.path.insert(0, ROOT)

OUT = os.path.join(ROOT, 'profiles', 'scene_time.json')
K_REF = np.array([[2257.7500557850776, 0, 1032], [0, 2257.4882391629421, 772], [0, 0, 1]])
H_REF, W_REF = 1544, 2064


def host_normals(P, radius, max_nn):
    """Hybrid search + covariance + eigh on the host, float64.  -> seconds, or None without scipy."""
    try:
        from scipy.spatial import cKDTree
    except ImportError:
        return None
    P = P.astype(np.float64)
    t0 = time.perf_counter()
    d, idx = cKDTree(P).query(P, k=max_nn, distance_upper_bound=radius, workers=-1)
    m = np.isfinite(d)
    pts = np.where(m[..., None], P[np.where(m, idx, 0)], 0.0)
    n = m.sum(axis=1, keepdims=True).astype(np.float64)
    dev = np.where(m[..., None], pts - (pts.sum(axis=1) / n)[:, None, :], 0.0)
    C = np.einsum('nki,nkj->nij', dev, dev) / n[:, :, None]
    np.linalg.eigh(C)
    return time.perf_counter() - t0


def main(reps, out_path, H, W):
    import torch
    from catgrasp_amd import _lib as L
    from catgrasp_amd import scene, synth
    from catgrasp_amd._lib import _p, _stream
    dev = torch.device('cuda:0')
    K = K_REF.copy()
    K[0, 2], K[1, 2] = K[0, 2] * W / W_REF, K[1, 2] * H / H_REF
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    radius, max_nn = 0.002, 30

    def timed(fn):
        fn(); torch.cuda.synchronize()
        ms = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); out = fn(); b.record(); torch.cuda.synchronize()
            ms.append(a.elapsed_time(b))
        return round(statistics.median(ms), 4), out

    depth = synth.make_depth_image(H, W, K, 60, seed=0)
    d_depth = torch.from_numpy(depth).to(dev)
    xyz = torch.empty((H, W, 3), dtype=torch.float32, device=dev)
    valid = torch.empty((H, W), dtype=torch.uint8, device=dev)
    normals = torch.empty((H, W, 3), dtype=torch.float64, device=dev)
    lib = L.lib()
    data = {'device': torch.cuda.get_device_name(0), 'reps': reps, 'image': [H, W], 'K': [fx, fy, cx, cy], 'radius': radius, 'max_nn': max_nn,
            'timer': 'HIP events, median'}
    data['depth_to_xyz_ms'], _ = timed(lambda: L.check(lib.cg_depth_to_xyz(_p(d_depth), 0, H, W, fx, fy, cx, cy, _p(xyz), _p(valid), _stream()), 'xyz'))
    use = valid.bool()
    hu, hv = scene.window_halfwidths(xyz, use, K, radius)
    fits = bool(lib.cg_scene_halo_fits(hu, hv))
    data.update(used_points=int(use.sum()), window_halfwidths=[hu, hv], auto_route='tiled' if fits else 'direct')
    # candidate evaluations of one scan: the clipped window of every used pixel
    z = xyz[..., 2].double() - radius
    wu = torch.ceil((fx + (torch.arange(W, device=dev).double() - cx).abs())[None, :] * radius / z) + 1
    wv = torch.ceil((fy + (torch.arange(H, device=dev).double() - cy).abs())[:, None] * radius / z) + 1
    uu, vv = torch.arange(W, device=dev).double()[None, :], torch.arange(H, device=dev).double()[:, None]
    nu = torch.minimum(uu + wu, torch.tensor(W - 1.0, device=dev)) - torch.maximum(uu - wu, torch.tensor(0.0, device=dev)) + 1
    nv = torch.minimum(vv + wv, torch.tensor(H - 1.0, device=dev)) - torch.maximum(vv - wv, torch.tensor(0.0, device=dev)) + 1
    cand = float((nu * nv)[use].sum())
    data['window_candidates_one_scan'] = cand
    count = torch.empty((H, W), dtype=torch.int32, device=dev)

    def run(route, cnt=None):
        L.check(lib.cg_organized_normals(_p(xyz), _p(valid), H, W, fx, fy, cx, cy, radius, max_nn, 0.0, 0.0, 0.0, route, hu, hv, _p(normals), _p(cnt),
                                         None, _stream()), 'normals')
        return normals
    for name, route in (('tiled', 1), ('direct', 2)):
        if route == 1 and not fits:
            continue
        data[f'organized_normals_{name}_ms'], out = timed(lambda: run(route))
        data[f'organized_normals_{name}_points_per_s'] = round(data['used_points'] / (data[f'organized_normals_{name}_ms'] * 1e-3))
        data[f'organized_normals_{name}_window_candidates_per_s'] = round(cand / (data[f'organized_normals_{name}_ms'] * 1e-3))
        if name == 'tiled':
            keep = out.clone()
        elif fits:
            data['routes_same_bits'] = bool(torch.equal(keep, out))
    run(0, count); torch.cuda.synchronize()
    c = count[use]
    data['neighbour_count'] = {'below_3': int((c < 3).sum()), 'below_max_nn': int((c < max_nn).sum()), 'at_max_nn': int((c == max_nn).sum())}
    data['scene_from_depth_ms'], front = timed(lambda: scene.scene_from_depth(depth, K, return_tensor=True))
    data['scene_pts'] = int(front['scene_pts'].shape[0])
    print(data, flush=True)

    # informational: the host doing the same search on a crop of about 100,000 points
    s = int(round(100000 ** 0.5))
    crop = xyz[H // 2 - s // 2:H // 2 - s // 2 + s, W // 2 - s // 2:W // 2 - s // 2 + s].reshape(-1, 3).cpu().numpy()
    sec = host_normals(crop, radius, max_nn)
    host = {'points': int(crop.shape[0]), 'what': 'scipy cKDTree.query(k=30, distance_upper_bound=radius, workers=-1) + numpy eigh, float64; informational',
            'cpus': os.cpu_count(), 'seconds': None if sec is None else round(sec, 3)}
    print(host, flush=True)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, 'w') as f:
        json.dump({'catgrasp_amd_on_mi355x': data, 'host_cpu_of_the_same_machine': host}, f, indent=1, sort_keys=True)
        f.write('\n')


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out', default=OUT)
    ap.add_argument('--height', type=int, default=H_REF)
    ap.add_argument('--width', type=int, default=W_REF)
    args = ap.parse_args()
    main(args.reps, args.out, args.height, args.width)
