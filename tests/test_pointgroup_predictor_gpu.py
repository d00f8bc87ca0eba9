"""GPU tests of predicter.PointGroupPredictor and pipeline.objects_from_scene on a synthetic bin of a few thousand points, with a seeded
synthetic checkpoint and the shipped settings in a temporary artifact directory."""
import os
import shutil

import numpy as np
import pytest
import torch

import pointgroup_ref as P
from catgrasp_amd import pipeline, pointgroup, segmentation, synth
from catgrasp_amd.aligning import voxel_down_sample_device
from catgrasp_amd.predicter import PointGroupPredictor

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
_CACHE = {}


def _scene():
    objs = synth.make_scene(3, 1200, seed=4, kind='nut')
    xyz, normal = np.concatenate([o['xyz'] for o in objs]), np.concatenate([o['normal'] for o in objs])
    perm = np.random.default_rng(5).permutation(len(xyz))
    return {'cloud_xyz': xyz[perm], 'cloud_normal': normal[perm], 'cloud_rgb': np.zeros_like(xyz)}


def _predictor(tmp_path_factory, dev):
    """One predictor per session: the yardstick's seeded weights with the last layer of the head scaled to millimetre offsets, saved the way
    the reference's training does ('state_dict' entry, DataParallel's 'module.' prefix)."""
    if 'p' not in _CACHE:
        d = tmp_path_factory.mktemp('artifacts') / 'artifacts-40'
        d.mkdir()
        shutil.copy(os.path.join(GOLDEN, 'config_pointgroup.yaml'), d / 'config_pointgroup.yaml')
        model = pointgroup.PointGroup(pointgroup.config_from_yaml(str(d / 'config_pointgroup.yaml')))
        sd = model.state_dict()
        sd.update({k: torch.from_numpy(v) for k, v in P.params().items()})
        sd['offset.3.weight'] = sd['offset.3.weight'] * 2e-3
        sd['offset.3.bias'] = sd['offset.3.bias'] * 2e-3
        torch.save({'state_dict': {'module.' + k: v for k, v in sd.items()}}, d / 'best_val.pth.tar')
        _CACHE['p'] = PointGroupPredictor('nut', root=str(d.parent), device=dev)
        _CACHE['dir'] = d
    return _CACHE['p']


def test_artifacts_are_found_or_named(tmp_path_factory, tmp_path, cuda_device):
    pred = _predictor(tmp_path_factory, cuda_device)
    assert pred.cfg_pg.m == 16 and pred.cfg['downsample_size'] == 0.0005 and not pred.model.training and pred.n_slice_per_side == 1
    assert next(pred.model.parameters()).is_cuda
    again = PointGroupPredictor('nut', artifact_dir=str(_CACHE['dir']), device=cuda_device)
    assert torch.equal(again.model.offset[3].weight, pred.model.offset[3].weight)
    with pytest.raises(FileNotFoundError, match='config_pointgroup.yaml'):
        PointGroupPredictor('nut', root=str(tmp_path), device=cuda_device)
    (tmp_path / 'artifacts-68').mkdir()
    shutil.copy(os.path.join(GOLDEN, 'config_pointgroup.yaml'), tmp_path / 'artifacts-68' / 'config_pointgroup.yaml')
    with pytest.raises(FileNotFoundError, match='best_val.pth.tar'):
        PointGroupPredictor('hnm', root=str(tmp_path), device=cuda_device)


def _voxelization_idx(locs):
    """numpy restatement of voxelization_idx, mode 4: voxels numbered by first appearance, rows [count, member ids ascending, 0 ...]."""
    table, members = {}, []
    p2v = np.empty(len(locs), dtype=np.int32)
    for i, row in enumerate(map(tuple, locs.tolist())):
        v = table.setdefault(row, len(table))
        if v == len(members):
            members.append([])
        members[v].append(i)
        p2v[i] = v
    width = max(len(m) for m in members)
    v2p = np.zeros((len(members), width + 1), dtype=np.int32)
    for v, m in enumerate(members):
        v2p[v, 0] = len(m)
        v2p[v, 1:1 + len(m)] = m
    return locs[[m[0] for m in members]], p2v, v2p


def test_front_end_against_a_numpy_restatement(tmp_path_factory, cuda_device):
    pred = _predictor(tmp_path_factory, cuda_device)
    data = _scene()
    fe = pred.front_end(data)
    cloud, normal = data['cloud_xyz'], data['cloud_normal']
    picks = fe['picks'][0].cpu().numpy()
    # every centroid's chosen point is A nearest point (a two-point voxel's midpoint is an exact tie)
    centroids = voxel_down_sample_device(torch.from_numpy(cloud).to(cuda_device), 0.0005).cpu().numpy()
    assert picks.shape == (len(centroids),) and 1000 < len(centroids) <= len(cloud)
    for s in range(0, len(centroids), 512):                                                # float64 brute force, a block of centroids at a time
        d2 = ((centroids[s:s + 512, None, :] - cloud[None, :, :]) ** 2).sum(-1)
        chosen = np.sqrt(d2[np.arange(d2.shape[0]), picks[s:s + 512]])
        assert (chosen <= np.sqrt(d2.min(1)) * (1 + 1e-12)).all()
    # given the picks, the rest is arithmetic
    xyz_origin = cloud[picks]
    xyz = xyz_origin * 500
    xyz -= xyz.min(0)
    locs = np.concatenate([np.zeros((len(xyz), 1), dtype=np.int64), xyz.astype(np.int64)], 1)
    assert np.array_equal(fe['locs'].cpu().numpy(), locs) and fe['locs'].dtype == torch.int64
    assert np.array_equal(fe['spatial_shape'], np.clip(locs.max(0)[1:] + 1, 128, None)) and fe['spatial_shape'].min() >= 128
    assert np.array_equal(fe['xyz_original'].cpu().numpy(), xyz_origin.astype(np.float32)) and fe['batch_offsets'].tolist() == [0, len(xyz)]
    voxel_coords, p2v, v2p = _voxelization_idx(locs)
    assert len(voxel_coords) < len(locs)                                                   # some voxels hold several points
    assert np.array_equal(fe['voxel_coords'].cpu().numpy(), voxel_coords) and np.array_equal(fe['p2v_map'].cpu().numpy(), p2v)
    assert np.array_equal(fe['v2p_map'].cpu().numpy(), v2p)
    point_feats = np.concatenate([normal[picks].astype(np.float32), xyz_origin.astype(np.float32)], 1).astype(np.float64)
    want = np.stack([point_feats[v2p[v, 1:1 + v2p[v, 0]]].mean(0) for v in range(len(v2p))])
    got = fe['voxel_feats'].cpu().numpy()
    assert got.shape == (len(v2p), 6) and np.abs(got - want).max() <= 1e-6


def test_labels_and_objects_from_a_scene(tmp_path_factory, cuda_device):
    pred = _predictor(tmp_path_factory, cuda_device)
    data = _scene()
    labels = pred.predict(data)
    assert labels.shape == (len(data['cloud_xyz']),) and labels.dtype == np.int64 and labels.min() >= 0
    assert pred.pt_offsets.shape == pred.xyz_original.shape and pred.pt_offsets.dtype == np.float32 and np.isfinite(pred.pt_offsets).all()
    assert np.abs(pred.pt_offsets).max() > 0 and pred.xyz_shifted.dtype == np.float32 and pred.xyz_shifted.shape[1] == 3
    want = segmentation.instances_from_offsets(data['cloud_xyz'], pred.xyz_original, pred.pt_offsets, class_name='nut')
    assert np.array_equal(labels, want) and 1 < len(np.unique(labels)) < len(labels)
    sizes = np.sort(np.bincount(labels))
    print(f'{len(np.unique(labels))} segments, the largest {sizes[-3:].tolist()}, offsets up to {np.abs(pred.pt_offsets).max():.3g} m')
    kw = dict(min_points=int(sizes[-2]), min_density=0.0)                                  # the offsets are no trained network's: keep the two largest
    cleaned, order = segmentation.select_segments(data['cloud_xyz'], labels, **kw)
    objects = pipeline.objects_from_scene(data, pred, **kw)
    assert len(objects) == len(order) >= 2
    for o, seg in zip(objects, order):
        assert np.array_equal(o['ob_pts'], data['cloud_xyz'][cleaned == seg]) and np.array_equal(o['ob_normals'], data['cloud_normal'][cleaned == seg])
