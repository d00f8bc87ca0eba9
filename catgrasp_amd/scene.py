"""The scene front end on the device: what the camera delivers -> the scene cloud the rest of the package starts from.

    depth image, K  ->  depth2xyzmap  ->  valid / background masks  ->  estimate_normals_organized  ->  data['cloud_xyz'], data['cloud_normal']

It replaces lines 192-212 and 245-250 of the reference's compute_candidate_grasp (run_grasp_simulation.py): depth2xyzmap, open3d's
estimate_normals(KDTreeSearchParamHybrid(radius=0.002, max_nn=30)), correct_pcd_normal_direction and the 1 mm voxel down-sampling of
the scene points.  The two kernels are csrc/scene.hip (ABI: include/catgrasp_amd_scene.h); masks and compaction are torch indexing
on the device.  The normals are those of an ORGANIZED cloud: the neighbours of a pixel's point are found in a pixel window around it,
which needs the camera matrix the map was made with.  Their semantics are stated in the header and restated in float64 numpy by
tests/scene_ref.py; they are not pinned against open3d."""
import math

import numpy as np
import torch

from . import _lib as L
from . import neighbors
from ._lib import _p, _stream, check
from .aligning import voxel_down_sample_device

ROUTES = {'auto': 0, 'tiled': 1, 'direct': 2}


def _device(*tensors, device=None):
    if device is not None:
        device = torch.device(device)
        if device.type != 'cuda':
            raise L.CatgraspAmdError('catgrasp_amd.scene needs a HIP device (no CPU fallback)')
        return device
    for t in tensors:
        if torch.is_tensor(t) and t.is_cuda:
            return t.device
    if not torch.cuda.is_available():
        raise L.CatgraspAmdError('catgrasp_amd.scene needs a HIP device (no CPU fallback)')
    return torch.device('cuda', torch.cuda.current_device())


def _intrinsics(K):
    """K -> (fx, fy, cx, cy) as Python floats; refuses anything but a finite 3 x 3 matrix with positive focal lengths."""
    k = K.detach().cpu().numpy() if torch.is_tensor(K) else np.asarray(K)
    if k.shape != (3, 3):
        raise ValueError(f'K must be a 3 x 3 camera matrix, got shape {k.shape}')
    k = k.astype(np.float64)
    fx, fy, cx, cy = float(k[0, 0]), float(k[1, 1]), float(k[0, 2]), float(k[1, 2])
    if not all(math.isfinite(x) for x in (fx, fy, cx, cy)) or fx <= 0 or fy <= 0:
        raise ValueError(f'K needs finite entries and positive fx, fy; got fx={fx}, fy={fy}, cx={cx}, cy={cy}')
    return fx, fy, cx, cy


def _host_tensor(a, what, dtypes):
    t = a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))
    if t.dtype not in dtypes:
        t = t.to(dtypes[-1])
    return t


def _mask(m, shape, what, device):
    t = m if torch.is_tensor(m) else torch.from_numpy(np.ascontiguousarray(m))
    if tuple(t.shape) != tuple(shape):
        raise ValueError(f'{what} must have the image\'s shape {tuple(shape)}, got {tuple(t.shape)}')
    return (t.to(device) != 0)


def _check_search(radius, max_nn):
    if not (isinstance(radius, (int, float, np.floating, np.integer)) and math.isfinite(radius) and radius > 0):
        raise ValueError(f'radius must be a positive finite number, got {radius!r}')
    if not isinstance(max_nn, (int, np.integer)) or int(max_nn) < 1:
        raise ValueError(f'max_nn must be an integer >= 1, got {max_nn!r}')


def depth2xyzmap(depth, K, device=None, return_valid=True):
    """Utils.depth2xyzmap on the device.  depth: (H, W) float32 or float64 array or tensor in metres (another dtype is taken as float64).
    -> xyz_map (H, W, 3) float32 device tensor, bit for bit the numpy function's; and, unless return_valid is False, the valid mask
    (H, W) bool: depth >= 0.1 in the depth's own dtype."""
    fx, fy, cx, cy = _intrinsics(K)
    d = _host_tensor(depth, 'depth', (torch.float32, torch.float64))
    if d.dim() != 2 or d.numel() == 0:
        raise ValueError(f'depth must be a non-empty (H, W) image, got shape {tuple(d.shape)}')
    if not bool(torch.isfinite(d).all()):
        raise ValueError('depth contains NaN or infinity')
    dev = _device(d, device=device)
    d = d.to(dev).contiguous()
    H, W = d.shape
    xyz = torch.empty((H, W, 3), dtype=torch.float32, device=dev)
    valid = torch.empty((H, W), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        check(L.lib().cg_depth_to_xyz(_p(d), int(d.dtype == torch.float64), H, W, fx, fy, cx, cy, _p(xyz), _p(valid), _stream()), 'cg_depth_to_xyz')
    return (xyz, valid.bool()) if return_valid else xyz


def window_halfwidths(xyz_map, use, K, radius):
    """The largest pixel half-widths (in u, in v) of the neighbour windows of the used pixels: per pixel
    ceil((fx + |u - cx|) * radius / (z - radius)) + 1, the whole image where z <= radius.  (0, 0) without a used pixel."""
    fx, fy, cx, cy = _intrinsics(K)
    H, W = use.shape
    z = xyz_map[..., 2].to(torch.float64) - radius
    big = float(max(H, W))
    au = fx + (torch.arange(W, device=use.device, dtype=torch.float64) - cx).abs()
    av = fy + (torch.arange(H, device=use.device, dtype=torch.float64) - cy).abs()
    zero = torch.zeros((), dtype=torch.float64, device=use.device)
    hu = torch.where(use, torch.where(z > 0, torch.ceil(au[None, :] * radius / z) + 1, big), zero).clamp(max=big)
    hv = torch.where(use, torch.where(z > 0, torch.ceil(av[:, None] * radius / z) + 1, big), zero).clamp(max=big)
    m = torch.stack((hu.max(), hv.max())).cpu()
    return int(m[0]), int(m[1])


def estimate_normals_organized(xyz_map, use, K, radius=0.002, max_nn=30, view_point=(0, 0, 0), route='auto', debug=False):
    """Oriented normals of an organized cloud: estimate_normals(KDTreeSearchParamHybrid(radius, max_nn)) + correct_pcd_normal_direction
    for every pixel of `use` (cg_organized_normals; semantics: include/catgrasp_amd_scene.h).  xyz_map: (H, W, 3) float32 device tensor as
    depth2xyzmap makes it with the same K; use: (H, W) mask.  -> normals (H, W, 3) float64, zero where `use` is false; with debug=True
    also the neighbour count (H, W) int32 and the largest neighbour d^2 (H, W) float64.  `route` ('auto', 'tiled', 'direct') exists
    for tests: the routes give identical bits; 'tiled' with a halo beyond the LDS budget raises."""
    fx, fy, cx, cy = _intrinsics(K)
    _check_search(radius, max_nn)
    vp = [float(x) for x in np.asarray(view_point, dtype=np.float64).reshape(-1)]
    if len(vp) != 3 or not all(math.isfinite(x) for x in vp):
        raise ValueError(f'view_point must be 3 finite numbers, got {view_point!r}')
    if route not in ROUTES:
        raise ValueError(f'route must be one of {sorted(ROUTES)}, got {route!r}')
    if not torch.is_tensor(xyz_map) or xyz_map.dim() != 3 or xyz_map.shape[2] != 3 or xyz_map.dtype != torch.float32:
        raise ValueError('xyz_map must be a (H, W, 3) float32 tensor')
    H, W = xyz_map.shape[:2]
    use_b = _mask(use, (H, W), 'use', xyz_map.device)
    L.require_cuda(xyz_map)
    dev = xyz_map.device
    xyz_map = xyz_map.contiguous()
    use_u8 = use_b.to(torch.uint8).contiguous()
    halo_u, halo_v = (0, 0) if route == 'direct' else window_halfwidths(xyz_map, use_b, K, float(radius))
    normals = torch.empty((H, W, 3), dtype=torch.float64, device=dev)
    count = torch.empty((H, W), dtype=torch.int32, device=dev) if debug else None
    d2max = torch.empty((H, W), dtype=torch.float64, device=dev) if debug else None
    with torch.cuda.device(dev):
        check(L.lib().cg_organized_normals(_p(xyz_map), _p(use_u8), H, W, fx, fy, cx, cy, float(radius), int(max_nn), vp[0], vp[1], vp[2],
                                           ROUTES[route], halo_u, halo_v, _p(normals), _p(count), _p(d2max), _stream()), 'cg_organized_normals')
    return (normals, count, d2max) if debug else normals


def scene_from_depth(depth, K, rgb=None, bg_mask=None, radius=0.002, max_nn=30, scene_voxel=0.001, return_tensor=False,
                     scene_normal_radius=None):
    """run_grasp_simulation.py:192-212 and :245-250 -> {'data': {'cloud_xyz', ['cloud_rgb',] 'cloud_normal'}, 'scene_pts'}.
    bg_mask: (H, W), non-zero for pixels that belong to the background (the reference marks the environment's bodies); invalid
    depth (< 0.1) is background by itself.  data['cloud_xyz']: float32 xyz_map[use] in row-major order, use = valid and not background;
    data['cloud_rgb']: rgb[use], only with `rgb` (H, W, 3); data['cloud_normal']: float64 oriented normals (radius, max_nn, view
    point at the camera).  scene_pts: the valid points voxel-down-sampled at `scene_voxel` (float64 centroids; colours are not
    averaged).  With scene_normal_radius (the reference's value is 0.003) the result also holds 'scene_normals': the oriented normals
    of scene_pts, an unorganized cloud, by neighbors.estimate_normals (run_grasp_simulation.py:247-248).  numpy arrays unless
    return_tensor."""
    _intrinsics(K)
    _check_search(radius, max_nn)
    if not (isinstance(scene_voxel, (int, float, np.floating, np.integer)) and math.isfinite(scene_voxel) and scene_voxel > 0):
        raise ValueError(f'scene_voxel must be a positive finite number, got {scene_voxel!r}')
    if scene_normal_radius is not None:
        _check_search(scene_normal_radius, max_nn)
    shape = tuple(depth.shape)
    if bg_mask is not None and tuple(bg_mask.shape) != shape:
        raise ValueError(f'bg_mask must have the image\'s shape {shape}, got {tuple(bg_mask.shape)}')
    if rgb is not None and tuple(rgb.shape[:2]) != shape:
        raise ValueError(f'rgb must have the image\'s shape {shape}, got {tuple(rgb.shape)}')
    xyz_map, valid = depth2xyzmap(depth, K)
    H, W = valid.shape
    dev = xyz_map.device
    use = valid if bg_mask is None else valid & ~_mask(bg_mask, (H, W), 'bg_mask', dev)
    colours = None
    if rgb is not None:
        colours = (rgb if torch.is_tensor(rgb) else torch.from_numpy(np.ascontiguousarray(rgb))).to(dev)[use]
    normals = estimate_normals_organized(xyz_map, use, K, radius=radius, max_nn=max_nn)
    data = {'cloud_xyz': xyz_map[use], 'cloud_normal': normals[use]}
    if colours is not None:
        data['cloud_rgb'] = colours
    scene_pts = voxel_down_sample_device(xyz_map[valid].to(torch.float64), float(scene_voxel))
    out = {'data': data, 'scene_pts': scene_pts}
    if scene_normal_radius is not None:
        out['scene_normals'] = neighbors.estimate_normals(scene_pts, radius=scene_normal_radius, max_nn=max_nn, return_tensor=True)
    if not return_tensor:
        out['data'] = {k: v.cpu().numpy() for k, v in data.items()}
        out.update({k: v.cpu().numpy() for k, v in out.items() if k != 'data'})
    return out
