"""CPU tests (no GPU) of the scene front end's restatement (tests/scene_ref.py): its depth2xyzmap is the reference function bit for bit,
the pixel window of cg_organized_normals leaves out no neighbour, the test scenes have the properties the GPU tests rest on, and
synth.make_depth_image intersects rays exactly."""
import os

import numpy as np
import pytest
import torch

import scene_ref as R
from catgrasp_amd import scene, synth

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'scene_golden.npz')


def test_restated_depth2xyzmap_is_the_reference_function_bit_for_bit():
    g = np.load(GOLDEN)
    for key in ('f32', 'f64'):
        depth, want = g['depth_' + key], g['xyz_' + key]
        assert depth.dtype == {'f32': np.float32, 'f64': np.float64}[key] and want.dtype == np.float32
        assert (depth < 0.1).any() and ((depth >= 0.1) & (depth < 0.10001)).any()       # both sides of the threshold are in the golden
        got, valid = R.depth2xyzmap(depth, g['K'])
        assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32))
        assert np.array_equal(valid, want[..., 2] != 0)


def _used_points(depth, bg, K):
    xyz, valid = R.depth2xyzmap(depth, K)
    use = valid if bg is None else valid & ~bg
    return xyz, use


@pytest.mark.parametrize('name', ['A', 'A_near', 'B'])
@pytest.mark.parametrize('radius', [0.002, 0.003])
def test_window_bound_excludes_no_in_range_neighbour(name, radius):
    depth, bg, K = {'A': (*R.scene_a(), R.K_A), 'A_near': (*R.scene_a(near_patch=True), R.K_A), 'B': (R.scene_b(), None, R.K_B)}[name]
    xyz, use = _used_points(depth, bg, K)
    q, j, _ = R.in_range_pairs(xyz[use], radius)
    hu, hv = R.window_halfwidths(xyz, K, radius)
    v, u = np.nonzero(use)
    assert len(q) > len(v)                                                              # there are neighbours besides the points themselves
    assert (np.abs(u[j] - u[q]) <= hu[use][q]).all() and (np.abs(v[j] - v[q]) <= hv[use][q]).all()
    # the package's own half-widths (what sizes the LDS halo) are the largest of these
    got = scene.window_halfwidths(torch.from_numpy(xyz), torch.from_numpy(use), K, radius)
    assert got == (int(hu[use].max()), int(hv[use].max()))
    if name == 'A' and radius == 0.002:
        assert got == (17, 17)
    if name == 'A_near':
        assert min(got) >= 39                                                           # beyond the LDS budget's 24


def test_scene_a_has_the_properties_its_gpu_test_rests_on():
    depth, bg = R.scene_a()
    xyz, use = _used_points(depth, bg, R.K_A)
    assert int(use.sum()) == 6551
    ref = R.organized_normals(xyz[use])
    c = ref['count']
    assert int((c < 3).sum()) == 1 and int(((c >= 3) & (c < 30)).sum()) > 500 and int((c == 30).sum()) > 5000
    assert int(ref['tie'].sum()) == 0
    ok = c >= 3
    assert ((ref['lam'][ok, 1] - ref['lam'][ok, 0]) / ref['lam'][ok, 2]).min() >= 1e-3
    assert np.abs((ref['view'] * ref['normals']).sum(axis=1)).min() >= 1e-6
    lone = int(np.nonzero(c < 3)[0][0])
    assert np.array_equal(ref['normals'][lone], np.array([0.0, 0.0, -1.0]) / (1 + 1e-10)) and xyz[use][lone, 2] == np.float32(0.30)


def test_scene_b_ties_are_exact_and_the_tie_rule_matters():
    xyz, use = _used_points(R.scene_b(), None, R.K_B)
    assert use.all()
    P = xyz[use]
    # every coordinate is exact in float32: the float64 products of the restatement are exact too
    u = np.arange(40)
    z = np.where(u % 3 == 0, 0.5 + 2.0 ** -12, 0.5)
    assert np.array_equal(xyz[7, :, 0].astype(np.float64), (u - 20) * z / 2048) and np.array_equal(xyz[7, :, 1].astype(np.float64), (7 - 20) * z / 2048)
    lo = R.organized_normals(P)
    hi = R.organized_normals(P, prefer='high', pairs=lo['pairs'])
    assert int(lo['tie'].sum()) >= 1400 and np.array_equal(lo['count'], hi['count']) and np.array_equal(lo['d2max'], hi['d2max'])
    inner = np.zeros((40, 40), bool)
    inner[10:30, 10:30] = True
    moved = np.abs(lo['normals'] - hi['normals']).max(axis=1)[inner.reshape(-1)]
    assert int((moved > 1e-6).sum()) == 400 and moved.max() > 0.05


def test_restated_normals_on_a_tilted_plane_and_the_selection_rule():
    # a noise-free plane z = z0 + a x + b y seen from the origin: every normal is the plane's, towards the camera
    H, W = 24, 28
    K = np.array([[2000.0, 0, 14], [0, 2000.0, 12], [0, 0, 1]])
    v, u = np.meshgrid(np.arange(H), np.arange(W), indexing='ij')
    rx, ry = (u - 14) / 2000.0, (v - 12) / 2000.0
    a, b, z0 = 0.3, -0.2, 0.5
    depth = z0 / (1 - a * rx - b * ry)
    xyz, valid = R.depth2xyzmap(depth, K)
    ref = R.organized_normals(xyz[valid])
    want = -np.array([-a, -b, 1.0]) / np.linalg.norm([a, b, 1.0])
    # float32 coordinates: z in [0.5, 1) is rounded by up to 2^-25 = 3e-8, over a patch of 30 points whose spread is about 3.7e-4 m
    # (pitch 2.5e-4): a tilt of at most 3e-8 / 3.7e-4 = 8e-5
    assert (ref['count'] == 30).all() and np.abs(ref['normals'] * (1 + 1e-10) - want).max() < 1e-4
    # the neighbour set is the max_nn nearest: its largest d2 is the 30th smallest of all squared distances
    P = xyz[valid].astype(np.float64)
    q = 300
    d2 = np.sort(((P - P[q]) ** 2).sum(axis=1))
    assert abs(ref['d2max'][q] - d2[29]) <= 1e-12 * d2[29] and d2[29] <= 0.002 ** 2


def test_make_depth_image_hits_plane_and_spheres_exactly():
    K = np.array([[2257.75, 0, 64], [0, 2257.49, 48], [0, 0, 1]])
    d = synth.make_depth_image(96, 128, K, 3, seed=1)
    assert d.shape == (96, 128) and d.dtype == np.float32 and np.isfinite(d).all() and d.min() > 0.4 and d.max() < 0.8
    assert np.array_equal(d, synth.make_depth_image(96, 128, K, 3, seed=1))
    flat = synth.make_depth_image(96, 128, K, 0, seed=1)
    xyz, _ = R.depth2xyzmap(flat, K)
    P = xyz.reshape(-1, 3).astype(np.float64)
    A = np.c_[P[:, :2], np.ones(len(P))]
    coef, *_ = np.linalg.lstsq(A, P[:, 2], rcond=None)
    assert np.abs(A @ coef - P[:, 2]).max() < 1e-6                                       # one plane, to float32 rounding
    assert (d <= flat).all() and (d < flat - 1e-3).sum() > 0                             # spheres only ever come nearer
