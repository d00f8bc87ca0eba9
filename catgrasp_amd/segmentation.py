"""The scene-to-objects step between the PointGroup network's offsets and `pipeline.evaluate_objects`:

  instances_from_offsets   the tail of PointGroupPredictor.predict (predicter.py:308-338) on the device
  select_segments          the segment selection of compute_candidate_grasp (run_grasp_simulation.py:217-263)

`pipeline.objects_from_segmentation` turns their result into the object list."""
import numpy as np
import torch

from . import _lib as L
from .aligning import voxel_down_sample_device
from .cluster import MeanShift, nearest_center

BANDWIDTH = {'hnm': 0.005, 'nut': 0.007, 'screw': 0.009}      # predicter.py:317-328
DOWNSAMPLE = 0.002                                            # predicter.py:309


def _dev(a, device, dtype=None):
    t = a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))
    return t.to(device=device, dtype=dtype).contiguous()


def instances_from_offsets(cloud_xyz, xyz_original, pt_offsets, class_name=None, bandwidth=None):
    """cloud_xyz (N,3): the scene points to label.  xyz_original (M,3) float32, pt_offsets (M,3) float32: the network's input points
    and its predicted offsets to the instance centers.  The bandwidth is BANDWIDTH[class_name] unless given.
    -> labels_all (N) int64 numpy.  The clustered cloud stays in `instances_from_offsets.xyz_shifted` (float32 numpy), as the
    reference keeps it in `self.xyz_shifted`.
    open3d's voxel_down_sample is restated by aligning.voxel_down_sample_device (not pinned against open3d)."""
    if bandwidth is None:
        if class_name not in BANDWIDTH:
            raise NotImplementedError(f'no MeanShift bandwidth for class {class_name!r} (known: {sorted(BANDWIDTH)})')
        bandwidth = BANDWIDTH[class_name]
    if not torch.cuda.is_available():
        raise L.CatgraspAmdError('catgrasp_amd.segmentation needs a HIP device (no CPU fallback)')
    dev = torch.device('cuda', torch.cuda.current_device())
    orig = _dev(xyz_original, dev, torch.float32)
    offs = _dev(pt_offsets, dev, torch.float32)
    orig64 = orig.double()
    down = voxel_down_sample_device(orig64, DOWNSAMPLE).contiguous()
    idx, _ = nearest_center(down, orig64)                     # cKDTree(xyz_original_all).query(xyz_down)
    xyz_down = orig[idx]
    xyz_shifted = xyz_down + offs[idx]
    ms = MeanShift(bandwidth=bandwidth, cluster_all=True, seeds=None).fit(xyz_shifted)
    idx_all, _ = nearest_center(_dev(cloud_xyz, dev, torch.float64), xyz_down.double().contiguous())
    instances_from_offsets.xyz_shifted = xyz_shifted.cpu().numpy()
    return ms._labels[idx_all].cpu().numpy()


def select_segments(cloud_xyz, labels, min_points=500, min_density=0.01):
    """-> (labels with every rejected segment set to -1, the surviving ids ordered for picking).  A segment is rejected with fewer
    than `min_points` points or with n / prod(extent / 1 mm) < min_density; the survivors are ordered by point count descending,
    among equal counts the larger id first (the reference reverses a stable ascending sort).  Counts and extents are torch
    reductions on the device the inputs are on (numpy input: the CPU); the outputs are numpy int64."""
    dev = cloud_xyz.device if torch.is_tensor(cloud_xyz) else labels.device if torch.is_tensor(labels) else torch.device('cpu')
    xyz = _dev(cloud_xyz, dev, torch.float64)
    lab = _dev(labels, dev, torch.int64)
    ids, inv = torch.unique(lab, return_inverse=True)         # ascending, like np.unique
    n = torch.bincount(inv, minlength=ids.shape[0])
    ix = inv.unsqueeze(1).expand(-1, 3)
    hi = torch.full((ids.shape[0], 3), -float('inf'), dtype=torch.float64, device=dev).scatter_reduce_(0, ix, xyz, 'amax')
    lo = torch.full((ids.shape[0], 3), float('inf'), dtype=torch.float64, device=dev).scatter_reduce_(0, ix, xyz, 'amin')
    density = n.double() / torch.prod((hi - lo) / 0.001, dim=1)
    ok = (ids >= 0) & (n >= min_points) & ~(density < min_density)
    cleaned = torch.where(ok[inv], lab, torch.full_like(lab, -1))
    ids_ok, n_ok = ids[ok], n[ok]
    order = ids_ok[torch.sort(n_ok, stable=True).indices].flip(0)
    return cleaned.cpu().numpy(), order.cpu().numpy()
