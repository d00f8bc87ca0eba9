"""GPU tests of the scene front end (csrc/scene.hip, catgrasp_amd/scene.py) against its float64 numpy restatement (tests/scene_ref.py).

Exact where the semantics are exact: the xyz map, the neighbour count and the largest neighbour d2 of every used pixel, zeros where a
pixel is not used, the default normal, and the equality of the routes.  The normals themselves are held to
    n^T C n - lambda_1 <= 1e-11 lambda_3      (C, lambda from the restatement: a two-pass float64 covariance of at most 30 terms errs by a
                                               few tens of 2^-53 trace(C), a stable solver adds the same order: about 1e-13 lambda_3)
    | |n| (1 + 1e-10) - 1 | <= 1e-12,  view . n >= 0
    | n - n_ref | <= 1e-9 componentwise       (Davis-Kahan: 2 |dC| / (lambda_2 - lambda_1) <= 6e-10 at the required gap ratio 1e-3)
at every used point; each scene asserts on the CPU side that it has the gap, the distance from ties and the |view . n| these need."""
import functools
import os

import numpy as np
import pytest
import torch

import scene_ref as R
from catgrasp_amd import _lib as L
from catgrasp_amd import pipeline, scene, segmentation
from catgrasp_amd.aligning import voxel_down_sample_device

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'scene_golden.npz')


@functools.lru_cache(maxsize=None)
def _scene(name):
    """-> depth, bg (or None), K, xyz_map, use of the restatement; shared and never written to."""
    depth, bg, K = {'A': lambda: (*R.scene_a(), R.K_A), 'A_near': lambda: (*R.scene_a(near_patch=True), R.K_A),
                    'B': lambda: (R.scene_b(), None, R.K_B)}[name]()
    xyz, valid = R.depth2xyzmap(depth, K)
    use = valid if bg is None else valid & ~bg
    return depth, bg, K, xyz, use


@functools.lru_cache(maxsize=None)
def _pairs(name, radius):
    xyz, use = _scene(name)[3:]
    return R.in_range_pairs(xyz[use], radius)


@functools.lru_cache(maxsize=None)
def _ref(name, radius=0.002, max_nn=30, prefer='low'):
    xyz, use = _scene(name)[3:]
    return R.organized_normals(xyz[use], radius, max_nn, prefer=prefer, pairs=_pairs(name, radius))


def _bits(a):
    return a.view(np.uint64) if a.dtype == np.float64 else a


def _run(name, dev, radius=0.002, max_nn=30, route='auto'):
    _, _, K, xyz, use = _scene(name)
    n, c, d = scene.estimate_normals_organized(torch.from_numpy(xyz).to(dev), torch.from_numpy(use).to(dev), K, radius=radius, max_nn=max_nn,
                                               route=route, debug=True)
    return n.cpu().numpy(), c.cpu().numpy(), d.cpu().numpy()


def _check_against(ref, use, normals, count, d2max, max_nn):
    """Every check of the module docstring, on every used point."""
    # the scene's own properties first (CPU side), so that the bars below cannot hide a failure
    ok = ref['count'] >= 3
    lam = ref['lam']
    if max_nn >= 3:
        assert int(ref['tie'].sum()) == 0
        assert ((lam[ok, 1] - lam[ok, 0]) / lam[ok, 2]).min() >= 1e-3
    assert np.abs((ref['view'] * ref['normals']).sum(axis=1)).min() >= 1e-6
    # exact
    assert np.array_equal(count[use], ref['count']) and np.array_equal(d2max[use].view(np.uint64), ref['d2max'].view(np.uint64))
    assert (normals[~use] == 0).all() and (count[~use] == 0).all()
    n = normals[use]
    few = ~ok
    assert np.array_equal(n[few], ref['normals'][few])                     # the default normal, oriented: the same bits
    # every used point
    rayleigh = np.einsum('ni,nij,nj->n', n, ref['C'], n) * (1 + 1e-10) ** 2
    print('max (n^T C n - l1) / l3', ((rayleigh - lam[:, 0])[ok] / lam[ok, 2]).max() if ok.any() else 0.0,
          'max |n - n_ref|', np.abs(n - ref['normals']).max())
    assert ((rayleigh - lam[:, 0])[ok] <= 1e-11 * lam[ok, 2]).all()
    assert (np.abs(np.linalg.norm(n, axis=1) * (1 + 1e-10) - 1) <= 1e-12).all()
    assert ((ref['view'] * n).sum(axis=1) >= 0).all()
    assert (np.abs(n - ref['normals']) <= 1e-9).all()


def test_depth2xyzmap_is_bit_equal_for_both_depth_dtypes(cuda_device):
    g = np.load(GOLDEN)
    cases = [(g['depth_f32'], g['K']), (g['depth_f64'], g['K'])]
    d32 = _scene('A')[0].copy()
    d64 = d32.astype(np.float64) + 1e-9                                    # float64 values that are no float32: the map rounds once
    f = np.float32(0.1)
    d32[0, :3] = [f, np.nextafter(f, np.float32(0)), np.nextafter(f, np.float32(1))]
    d64[0, :4] = [0.1, np.nextafter(0.1, 0), np.nextafter(0.1, 1), float(f)]
    cases += [(d32, R.K_A), (d64, R.K_A)]
    for depth, K in cases:
        assert (depth < 0.1).any() and ((depth >= 0.1) & (depth < 0.11)).any()
        want, valid = R.depth2xyzmap(depth, K)
        xyz, got_valid = scene.depth2xyzmap(depth, K, device=cuda_device)
        assert xyz.dtype == torch.float32 and xyz.is_cuda and got_valid.dtype == torch.bool
        assert np.array_equal(xyz.cpu().numpy().view(np.uint32), want.view(np.uint32)) and np.array_equal(got_valid.cpu().numpy(), valid)
        only = scene.depth2xyzmap(torch.from_numpy(depth).to(cuda_device), K, return_valid=False)
        assert torch.equal(only, xyz)
    assert np.array_equal(scene.depth2xyzmap(g['depth_f32'], g['K'])[0].cpu().numpy().view(np.uint32), g['xyz_f32'].view(np.uint32))


@pytest.mark.parametrize('radius,max_nn', [(0.002, 30), (0.003, 30), (0.002, 1), (0.002, 2), (0.002, 500)])
def test_scene_a_normals_counts_and_d2max(cuda_device, radius, max_nn):
    use = _scene('A')[4]
    ref = _ref('A', radius, max_nn)
    normals, count, d2max = _run('A', cuda_device, radius, max_nn)
    _check_against(ref, use, normals, count, d2max, max_nn)
    c = ref['count']
    if (radius, max_nn) == (0.002, 30):
        assert len(c) == 6551 and int((c < 3).sum()) == 1 and int(((c >= 3) & (c < 30)).sum()) > 500 and int((c == 30).sum()) > 5000
        lone = normals[5, 80]                                              # the pixel at z = 0.30
        assert count[5, 80] == 1 and np.array_equal(lone, np.array([0.0, 0.0, -1.0]) / (1 + 1e-10))
    if max_nn < 3:                                                         # every normal is the default one, towards the camera
        assert np.array_equal(normals[use], np.tile(np.array([0.0, 0.0, -1.0]) / (1 + 1e-10), (len(c), 1)))
    if max_nn == 500:                                                      # nothing is capped
        q = _pairs('A', radius)[0]
        assert np.array_equal(c, np.bincount(q, minlength=len(c))) and c.max() > 60


def test_scene_b_exact_ties_go_to_the_smaller_pixel_index(cuda_device):
    use = _scene('B')[4]
    lo, hi = _ref('B'), _ref('B', prefer='high')
    inner = np.zeros((40, 40), bool)
    inner[10:30, 10:30] = True
    # CPU side: ties are there, and the opposite rule would fail the componentwise bar at the interior points
    assert int(lo['tie'].sum()) >= 1400
    assert int((np.abs(hi['normals'] - lo['normals']).max(axis=1)[inner.reshape(-1)] > 1e-9).sum()) >= 100
    normals, count, d2max = _run('B', cuda_device)
    assert np.array_equal(count[use], lo['count']) and np.array_equal(d2max[use].view(np.uint64), lo['d2max'].view(np.uint64))
    assert (np.abs(normals[use] - lo['normals']) <= 1e-9).all()
    n = normals[use]
    rayleigh = np.einsum('ni,nij,nj->n', n, lo['C'], n) * (1 + 1e-10) ** 2
    assert ((rayleigh - lo['lam'][:, 0]) <= 1e-11 * lo['lam'][:, 2]).all()


def _direct_call(xyz, use, K, halo, route, radius=0.002, max_nn=30):
    """cg_organized_normals with a halo of the test's choosing (the Python front always passes the largest window)."""
    H, W = use.shape
    n = torch.empty((H, W, 3), dtype=torch.float64, device=xyz.device)
    c = torch.empty((H, W), dtype=torch.int32, device=xyz.device)
    d = torch.empty((H, W), dtype=torch.float64, device=xyz.device)
    st = L.lib().cg_organized_normals(L._p(xyz), L._p(use), H, W, K[0, 0], K[1, 1], K[0, 2], K[1, 2], radius, max_nn, 0.0, 0.0, 0.0, route, halo[0],
                                      halo[1], L._p(n), L._p(c), L._p(d), L._stream())
    return st, n, c, d


@pytest.mark.parametrize('name', ['A', 'B'])
def test_routes_and_halos_give_the_same_bits(cuda_device, name):
    _, _, K, xyz, use = _scene(name)
    tiled, direct, auto = (_run(name, cuda_device, route=r) for r in ('tiled', 'direct', 'auto'))
    for a, b, c in zip(tiled, direct, auto):
        assert np.array_equal(_bits(a), _bits(b)) and np.array_equal(_bits(a), _bits(c))
    # a halo smaller than some windows: those queries read global memory inside the tiled kernel, and nothing changes
    d_xyz, d_use = torch.from_numpy(xyz).to(cuda_device), torch.from_numpy(use.astype(np.uint8)).to(cuda_device)
    for halo in ((8, 8), (0, 0), (3, 11), (24, 24)):
        st, n, c, d = _direct_call(d_xyz, d_use, K, halo, 1)
        assert st == 0
        assert np.array_equal(n.cpu().numpy().view(np.uint64), direct[0].view(np.uint64)) and np.array_equal(c.cpu().numpy(), direct[1])
        assert np.array_equal(d.cpu().numpy().view(np.uint64), direct[2].view(np.uint64))


def test_a_near_patch_sends_auto_to_direct_and_refuses_forced_tiled(cuda_device):
    _, _, K, xyz, use = _scene('A_near')
    hw = scene.window_halfwidths(torch.from_numpy(xyz), torch.from_numpy(use), K, 0.002)
    assert min(hw) >= 39 and L.lib().cg_scene_halo_fits(*hw) == 0          # about 40 pixels: beyond the 64 KiB budget
    auto, direct = _run('A_near', cuda_device, route='auto'), _run('A_near', cuda_device, route='direct')
    for a, b in zip(auto, direct):
        assert np.array_equal(_bits(a), _bits(b))
    with pytest.raises(L.CatgraspAmdError, match='status -1'):
        _run('A_near', cuda_device, route='tiled')
    d_xyz, d_use = torch.from_numpy(xyz).to(cuda_device), torch.from_numpy(use.astype(np.uint8)).to(cuda_device)
    assert _direct_call(d_xyz, d_use, K, hw, 1)[0] == -1                   # CG_ERR_ARG from C, nothing launched
    _check_against(_ref('A_near'), use, *direct, 30)                       # the 40-pixel windows find what brute force finds


def test_cropping_by_offsets_that_are_no_multiple_of_the_tile_changes_no_bit(cuda_device):
    depth, bg = _scene('A')[:2]
    K = R.K_A.copy()
    K[0, 2], K[1, 2] = 40.0, 31.0                                          # an integer principal point: u - cx is the same number after the crop
    top, left, bottom, right = 5, 7, 66, 89
    Kc = K.copy()
    Kc[0, 2], Kc[1, 2] = K[0, 2] - left, K[1, 2] - top
    xyz, valid = R.depth2xyzmap(depth, K)
    xyz_c, valid_c = R.depth2xyzmap(depth[top:bottom, left:right].copy(), Kc)
    assert np.array_equal(xyz[top:bottom, left:right].view(np.uint32), xyz_c.view(np.uint32))
    use, use_c = valid & ~bg, valid_c & ~bg[top:bottom, left:right]
    full = scene.estimate_normals_organized(torch.from_numpy(xyz).to(cuda_device), torch.from_numpy(use).to(cuda_device), K, debug=True)
    crop = scene.estimate_normals_organized(torch.from_numpy(xyz_c).to(cuda_device), torch.from_numpy(use_c).to(cuda_device), Kc, debug=True)
    hu, hv = R.window_halfwidths(xyz, K, 0.002)
    v, u = np.meshgrid(np.arange(72), np.arange(96), indexing='ij')
    inside = use & (u - hu >= left) & (u + hu < right) & (v - hv >= top) & (v + hv < bottom)
    assert int(inside.sum()) > 2000
    m = inside[top:bottom, left:right]
    for f, c in zip(full, crop):
        f, c = f.cpu().numpy()[top:bottom, left:right][m], c.cpu().numpy()[m]
        assert np.array_equal(_bits(f), _bits(c))


def test_scene_from_depth_assembles_the_scene_cloud(cuda_device):
    depth, bg, K, xyz, use = _scene('A')
    valid = depth >= np.float32(0.1)
    rgb = np.random.default_rng(5).integers(0, 256, (72, 96, 3), dtype=np.uint8)
    out = scene.scene_from_depth(depth, K, rgb=rgb, bg_mask=bg, return_tensor=True)
    data = out['data']
    assert sorted(data) == ['cloud_normal', 'cloud_rgb', 'cloud_xyz']
    assert data['cloud_xyz'].dtype == torch.float32 and np.array_equal(data['cloud_xyz'].cpu().numpy().view(np.uint32), xyz[use].view(np.uint32))
    assert np.array_equal(data['cloud_rgb'].cpu().numpy(), rgb[use])
    n = data['cloud_normal'].cpu().numpy()
    ref = _ref('A')
    assert n.dtype == np.float64 and (np.abs(n - ref['normals']) <= 1e-9).all()
    assert (np.abs(np.linalg.norm(n, axis=1) * (1 + 1e-10) - 1) <= 1e-12).all() and ((ref['view'] * n).sum(axis=1) >= 0).all()
    want_pts = voxel_down_sample_device(torch.from_numpy(xyz[valid]).to(cuda_device).to(torch.float64), 0.001)
    assert torch.equal(out['scene_pts'], want_pts) and 0 < len(want_pts) < int(valid.sum())
    # numpy out by default, no colours without rgb, and a tensor depth on the device is taken as it is
    plain = scene.scene_from_depth(torch.from_numpy(depth).to(cuda_device), K, bg_mask=torch.from_numpy(bg))
    assert sorted(plain['data']) == ['cloud_normal', 'cloud_xyz'] and isinstance(plain['scene_pts'], np.ndarray)
    assert np.array_equal(plain['data']['cloud_xyz'], xyz[use]) and np.array_equal(plain['data']['cloud_normal'], n)
    assert np.array_equal(plain['scene_pts'], want_pts.cpu().numpy())
    # without a background mask every valid pixel is used
    assert len(scene.scene_from_depth(depth, K)['data']['cloud_xyz']) == int(valid.sum())


class _BlockPredictor:
    """Stands in for PointGroupPredictor: labels by quarter of the cloud's x range; needs no checkpoint."""

    def predict(self, data):
        self.data = data
        x = np.asarray(data['cloud_xyz'])[:, 0]
        return np.digitize(x, np.quantile(x, [0.2, 0.5, 0.9])).astype(np.int64)


def test_objects_from_depth_runs_the_front_end_and_then_the_segment_selection(cuda_device):
    depth, bg, K, xyz, use = _scene('A')
    stub = _BlockPredictor()
    kw = dict(min_points=1000, min_density=0.0)
    objects, scene_pts = pipeline.objects_from_depth(depth, K, stub, bg_mask=bg, **kw)
    front = scene.scene_from_depth(depth, K, bg_mask=bg)
    assert np.array_equal(stub.data['cloud_xyz'], xyz[use]) and np.array_equal(scene_pts, front['scene_pts'])
    labels = stub.predict(front['data'])
    cleaned, order = segmentation.select_segments(front['data']['cloud_xyz'], labels, **kw)
    want = pipeline.objects_from_segmentation(front['data']['cloud_xyz'], front['data']['cloud_normal'], cleaned, order)
    assert order.tolist() == [2, 1, 0] and len(objects) == 3               # the last tenth is below min_points
    for o, w in zip(objects, want):
        assert np.array_equal(o['ob_pts'], w['ob_pts']) and np.array_equal(o['ob_normals'], w['ob_normals'])
        assert o['ob_pts'].dtype == np.float32 and o['ob_normals'].dtype == np.float64 and len(o['ob_pts']) >= 1000
