"""GPU parity of the SDF lookups (meshpy Sdf3D restatement in oracle/sdf_ref.py)."""
import os

import numpy as np
import pytest
import torch

from oracle import sdf_ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def box():
    data, origin, res = sdf_ref.box_sdf_grid([-0.01, -0.004, -0.007], [0.012, 0.006, 0.003], 0.001, 5)
    return data, origin, res


def test_trilinear_nearest_and_inside(cuda_device, box, tmp_path):
    from catgrasp_amd.sdf import Sdf3D, SdfFile
    data, origin, res = box
    sdf = Sdf3D(data, origin, res, device=cuda_device)
    rng = np.random.default_rng(0)
    n = 20000
    coords = rng.uniform(-3, data.shape[0] + 3, (3, n))            # includes out-of-grid points (clipped)
    coords[:, :200] = np.round(coords[:, :200]) + 0.5              # exact .5 -> round-half-even matters
    coords[:, 200:300] = np.round(coords[:, 200:300])              # exact lattice points
    c32 = coords.astype(np.float32).astype(np.float64)             # the device sees float32 coordinates
    got = sdf._signed_distance(c32).cpu().numpy()
    ref = sdf_ref.signed_distance(data, c32)
    assert np.abs(got - ref).max() <= 1e-4 * np.abs(data).max() * 1e-2 + 2e-7       # float32 weights vs float64
    got_fast = sdf._signed_distance(c32, fast=True).cpu().numpy()
    assert np.array_equal(got_fast, sdf_ref.signed_distance(data, c32, fast=True).astype(np.float32))
    cb = np.stack([c32[:, :5000], c32[:, 5000:10000]])
    gb = sdf._signed_distance_batch(torch.from_numpy(cb).float().to(cuda_device)).cpu().numpy()
    assert np.array_equal(gb, sdf_ref.signed_distance_batch(data, cb).astype(np.float32))
    with pytest.raises(NotImplementedError):
        sdf._signed_distance_batch(torch.zeros(1, 3, 4), fast=False)
    # any-inside: all-outside cloud, one inside point, points beyond the grid are dropped not clamped
    centre_grid = sdf.transform_pt_obj_to_grid(np.array([[0.001], [0.001], [-0.002]]))
    assert sdf.is_any_points_inside(centre_grid) and sdf_ref.is_any_points_inside(data, centre_grid)
    far = np.array([[-50.0, 500.0], [3.0, 3.0], [3.0, 3.0]])
    assert not sdf.is_any_points_inside(far) and not sdf_ref.is_any_points_inside(data, far)
    for _ in range(20):
        c = rng.uniform(-5, data.shape[0] + 5, (3, 50))
        assert sdf.is_any_points_inside(c.astype(np.float32)) == sdf_ref.is_any_points_inside(data, c.astype(np.float32))
    # SdfFile round trip (x fastest, z slowest in the file; data[i][j][k] in memory)
    path = os.path.join(tmp_path, 'box.sdf')
    small = data[:7, :6, :5]
    SdfFile.write(path, small, origin, res)
    d2, o2, r2 = sdf_ref.read_sdf_file(path)
    s2 = SdfFile(path).read(device=cuda_device)
    assert np.array_equal(d2, small) and np.array_equal(s2.data_torch.cpu().numpy(), small.astype(np.float32))
    assert np.allclose(s2.origin, o2) and s2.resolution == r2
    assert SdfFile(os.path.join(tmp_path, 'missing.sdf')).read() is None


def test_batched_candidate_inside_check(cuda_device, box):
    """Sdf3D.is_any_points_inside_batch against the float64 oracle.  The device composes the transform in float32, so a point within
    the coordinate bound of a rounding boundary may land in the neighbouring voxel; prep_ref.sdf_classify finds from float64 alone
    which candidates that can flip.  Every candidate float64 forces must agree, and at most 1 % may be undecided (none is, for
    these inputs: tests/test_prep_ref_cpu.py)."""
    import prep_ref as Q
    from catgrasp_amd.sdf import Sdf3D
    data, origin, res = box
    sdf = Sdf3D(data, origin, res, device=cuda_device)
    for E, sigma, seed in ((64, 0.03, 1), (500, 0.02, 3)):
        poses, pts = Q.sdf_pose_case(E, sigma, seed)
        got = sdf.is_any_points_inside_batch(poses, pts).cpu().numpy()
        cls, exp = Q.sdf_classify(data, sdf.T_world_grid, poses, pts)
        und = Q.check_sdf_batch(got, cls, f'E {E} sigma {sigma}')
        print(f'E {E} sigma {sigma}: {und} undecided, {int((got != exp).sum())} differ from the oracle, inside share {exp.mean():.3f}')
        assert 0 < exp.sum() < len(exp)


def test_robot_gripper_loads_sdf_grids_onto_the_device(cuda_device, box, tmp_path):
    """RobotGripper.load (dexnet/grasping/gripper.py:119-129): the optional .sdf files next to the meshes become device Sdf3D grids."""
    from catgrasp_amd import gripper as G
    from catgrasp_amd import synth
    from catgrasp_amd.sdf import SdfFile
    data, origin, res = box
    g = synth.make_gripper()
    d = str(tmp_path)
    G.save_obj(f'{d}/gripper_air_tight.obj', g['vertices'], g['faces'])
    G.save_obj(f'{d}/gripper_enclosed_air_tight.obj', g['enclosed_vertices'], g['enclosed_faces'])
    G.save_obj(f'{d}/finger1.obj', *synth.box_mesh([0.0, 0.02, -0.01], [0.04, 0.03, 0.01]))
    open(f'{d}/params.json', 'w').write('{"hand_depth": 0.04}')
    G.save_rigid_transform(f'{d}/T_grasp_gripper.tf', np.linalg.inv(g['gripper_in_grasp']), 'gripper', 'grasp')
    small = data[:9, :8, :7]
    SdfFile.write(f'{d}/gripper_air_tight.sdf', small, origin, res)
    rg = G.RobotGripper.load(d, device=cuda_device)
    assert rg.sdf is not None and rg.sdf_enclosed is None
    assert np.array_equal(rg.sdf.data_torch.cpu().numpy(), small.astype(np.float32)) and rg.sdf.data_torch.is_cuda
    c = np.array([[1.5], [2.25], [3.0]])
    assert abs(float(rg.sdf._signed_distance(c).cpu()[0]) - sdf_ref.signed_distance(small, c)[0]) < 1e-6
