"""A grid index on the device: radius-bounded neighbour queries and oriented normals for ANY point cloud.

    points  ->  GridIndex(points, cell)  ->  .estimate_normals(radius, max_nn)      open3d estimate_normals(KDTreeSearchParamHybrid) +
                                                                                     correct_pcd_normal_direction (Utils.py:205-213)
                                             .nearest_within(query, radius)          cKDTree.query(k=1, distance_upper_bound=radius)
                                             .count_within(query, radius)            cKDTree.query_ball_point(..., return_length=True)

scene.estimate_normals_organized needs the depth image's pixel grid; this needs nothing but the points: a cloud fused from several
views, a cropped or down-sampled one, the reference's 1 mm `scene_pts` (run_grasp_simulation.py:247-248).  The index is a uniform
lattice of `cell`-sized cells (cell >= radius): one 63-bit key per point, the points sorted by (key, index) with torch's stable device
sort, a query answered from the few cells around it (csrc/grid_index.hip; ABI and semantics: include/catgrasp_amd_neighbors.h).  The
cells only decide where the kernels look: no result depends on `cell`.  The normals have the pinned semantics of
cg_organized_normals with "pixel index" read as "point index" and share its code after the search, so on a depth image's used points
they are the same bits (tests/test_neighbors_gpu.py)."""
import math
import sys

import numpy as np
import torch

from . import _lib as L
from ._lib import _p, _stream, check

MAX_NN = 64                                                   # CG_NB_MAX_NN of the header


def _device(*tensors, device=None):
    if device is not None:
        device = torch.device(device)
        if device.type != 'cuda':
            raise L.CatgraspAmdError('catgrasp_amd.neighbors needs a HIP device (no CPU fallback)')
        return device
    for t in tensors:
        if torch.is_tensor(t) and t.is_cuda:
            return t.device
    if not torch.cuda.is_available():
        raise L.CatgraspAmdError('catgrasp_amd.neighbors needs a HIP device (no CPU fallback)')
    return torch.device('cuda', torch.cuda.current_device())


def _positive(x, what):
    if not (isinstance(x, (int, float, np.floating, np.integer)) and not isinstance(x, bool) and math.isfinite(x) and x > 0):
        raise ValueError(f'{what} must be a positive finite number, got {x!r}')
    return float(x)


def _cloud(a, what):
    """-> (n, 3) float32 or float64 tensor with finite entries, wherever it lives (another dtype is taken as float64)."""
    if not torch.is_tensor(a):
        a = np.ascontiguousarray(a)
        a = torch.from_numpy(a if a.flags.writeable else a.copy())          # never written to; torch only warns about read-only memory
    t = a
    if t.dim() != 2 or t.shape[1] != 3:
        raise ValueError(f'{what} must have shape (n, 3), got {tuple(t.shape)}')
    if t.dtype not in (torch.float32, torch.float64):
        t = t.to(torch.float64)
    if t.numel() and not bool(torch.isfinite(t).all()):
        raise ValueError(f'{what} contains NaN or infinity')
    return t.detach()


def _status(status, what):
    if status == -2:
        raise NotImplementedError(f'{what}: beyond a limit of the kernel contract (include/catgrasp_amd_neighbors.h)')
    check(status, what)


class GridIndex:
    """The index of one cloud.  points: (N, 3) float32 or float64, array or tensor; cell: the lattice pitch, at least the largest radius
    that will be asked.  Building it is one key kernel, one stable sort and two gathers on the device."""

    def __init__(self, points, cell, device=None):
        self.cell = _positive(cell, 'cell')
        pts = _cloud(points, 'points')
        self.device = _device(pts, device=device)
        self.n = int(pts.shape[0])
        if self.n >= 2 ** 31:
            raise NotImplementedError('GridIndex: point indices are int32')
        if self.n == 0:
            return
        pts = pts.to(self.device).contiguous()
        p64 = pts.to(torch.float64)
        box = torch.stack((p64.min(dim=0).values, p64.max(dim=0).values)).cpu().tolist()
        self.origin = box[0]
        self.ext = [int(math.floor((hi - lo) / self.cell)) + 1 for lo, hi in zip(*box)]
        if self.ext[0] * self.ext[1] * self.ext[2] >= 2 ** 62:
            raise ValueError('GridIndex: the cell lattice of this cloud does not fit 62 bits (cell too small)')
        keys = torch.empty((self.n,), dtype=torch.int64, device=self.device)
        with torch.cuda.device(self.device):
            _status(L.lib().cg_grid_cell_keys(_p(pts), int(pts.dtype == torch.float64), self.n, *self.origin, self.cell, *self.ext, _p(keys),
                                              _stream()), 'cg_grid_cell_keys')
        self.sorted_keys, order = torch.sort(keys, stable=True)        # by (key, original index)
        self.sorted_points = p64[order].contiguous()
        self.sorted_index = order.to(torch.int32)

    def _grid(self):
        return (_p(self.sorted_points), _p(self.sorted_index), _p(self.sorted_keys), self.n, *self.origin, self.cell, *self.ext)

    def _radius(self, radius):
        radius = self.cell if radius is None else _positive(radius, 'radius')
        if radius > self.cell:
            raise ValueError(f'radius {radius!r} exceeds the index\'s cell {self.cell!r}: build the GridIndex with cell >= radius')
        if radius * radius < sys.float_info.min:
            raise ValueError(f'radius {radius!r} is too small: its square is no normal float64')
        return radius

    def estimate_normals(self, radius=None, max_nn=30, view_point=(0, 0, 0), debug=False):
        """Oriented normals of the indexed points (cg_grid_normals), in the points' own order: (N, 3) float64 device tensor; with debug=True
        also the neighbour count (N) int32 and the largest neighbour d^2 (N) float64.  radius defaults to the cell."""
        radius = self._radius(radius)
        if not isinstance(max_nn, (int, np.integer)) or isinstance(max_nn, bool) or int(max_nn) < 1:
            raise ValueError(f'max_nn must be an integer >= 1, got {max_nn!r}')
        if int(max_nn) > MAX_NN:
            raise NotImplementedError(f'max_nn = {max_nn} exceeds CG_NB_MAX_NN = {MAX_NN} (the reference uses 30 at every call)')
        vp = [float(x) for x in np.asarray(view_point, dtype=np.float64).reshape(-1)]
        if len(vp) != 3 or not all(math.isfinite(x) for x in vp):
            raise ValueError(f'view_point must be 3 finite numbers, got {view_point!r}')
        normals = torch.empty((self.n, 3), dtype=torch.float64, device=self.device)
        count = torch.empty((self.n,), dtype=torch.int32, device=self.device) if debug else None
        d2max = torch.empty((self.n,), dtype=torch.float64, device=self.device) if debug else None
        if self.n:
            with torch.cuda.device(self.device):
                _status(L.lib().cg_grid_normals(*self._grid(), radius, int(max_nn), *vp, _p(normals), _p(count), _p(d2max), _stream()),
                        'cg_grid_normals')
        return (normals, count, d2max) if debug else normals

    def _queries(self, query):
        """-> the queries on the device and the order that walks them cell by cell (None without a point or a query)."""
        q = _cloud(query, 'query').to(self.device).contiguous()
        m = int(q.shape[0])
        if m >= 2 ** 31:
            raise NotImplementedError('GridIndex: query indices are int32')
        if m == 0 or self.n == 0:
            return q, m, None
        keys = torch.empty((m,), dtype=torch.int64, device=self.device)
        with torch.cuda.device(self.device):
            _status(L.lib().cg_grid_cell_keys(_p(q), int(q.dtype == torch.float64), m, *self.origin, self.cell, *self.ext, _p(keys), _stream()),
                    'cg_grid_cell_keys')
        return q, m, torch.sort(keys, stable=True).indices.to(torch.int32)

    def nearest_within(self, query, radius):
        """Per query point the closest indexed point within `radius` (cg_grid_nearest_within) -> (index (M) int32, -1 where there is none;
        d^2 (M) float64, +inf there).  Exact ties go to the smaller index."""
        radius = self._radius(radius)
        q, m, order = self._queries(query)
        idx = torch.full((m,), -1, dtype=torch.int32, device=self.device)
        d2 = torch.full((m,), math.inf, dtype=torch.float64, device=self.device)
        if order is not None:
            with torch.cuda.device(self.device):
                _status(L.lib().cg_grid_nearest_within(*self._grid(), _p(q), int(q.dtype == torch.float64), _p(order), m, radius, _p(idx), _p(d2),
                                                       _stream()), 'cg_grid_nearest_within')
        return idx, d2

    def count_within(self, query, radius):
        """Per query point the number of indexed points within `radius` (cg_grid_count_within) -> (M) int32."""
        radius = self._radius(radius)
        q, m, order = self._queries(query)
        count = torch.zeros((m,), dtype=torch.int32, device=self.device)
        if order is not None:
            with torch.cuda.device(self.device):
                _status(L.lib().cg_grid_count_within(*self._grid(), _p(q), int(q.dtype == torch.float64), _p(order), m, radius, _p(count),
                                                     _stream()), 'cg_grid_count_within')
        return count


def estimate_normals(xyz, radius=0.002, max_nn=30, view_point=(0, 0, 0), device=None, return_tensor=False, debug=False):
    """open3d's estimate_normals(KDTreeSearchParamHybrid(radius, max_nn)) + correct_pcd_normal_direction for an unorganized cloud.
    xyz: (N, 3) float32 or float64.  -> (N, 3) float64 normals, a numpy array unless return_tensor; with debug=True also the neighbour
    count and the largest neighbour d^2."""
    out = GridIndex(xyz, _positive(radius, 'radius'), device=device).estimate_normals(radius, max_nn, view_point, debug=debug)
    if return_tensor:
        return out
    return tuple(o.cpu().numpy() for o in out) if debug else out.cpu().numpy()


def cloudA_minus_cloudB(ptsA, ptsB, thres, device=None):
    """Utils.cloudA_minus_cloudB: the points of A without a point of B within `thres` -> (ptsA[keep_ids], keep_ids), keep_ids ascending."""
    thres = _positive(thres, 'thres')
    a, b = _cloud(ptsA, 'ptsA'), _cloud(ptsB, 'ptsB')
    count = GridIndex(b, thres, device=_device(a, b, device=device)).count_within(a, thres)
    keep = torch.nonzero(count == 0).reshape(-1)
    if torch.is_tensor(ptsA):
        return ptsA[keep.to(ptsA.device)], keep
    keep = keep.cpu().numpy()
    return np.asarray(ptsA)[keep], keep
