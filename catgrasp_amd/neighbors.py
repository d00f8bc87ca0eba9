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
they are the same bits (tests/test_neighbors_gpu.py).

                                             .nearest(query)                         cKDTree.query(x), no distance_upper_bound
                                             .ball_point(query, radius)              cKDTree.query_ball_point(x, r)
    data    ->  cKDTree(data)            ->  .query(x) / .query_ball_point(x, r)     scipy.spatial.cKDTree at the reference's call shapes

The unbounded nearest neighbour (include/catgrasp_amd_kdtree.h) searches boxes of doubling radius around the query and is exact:
index for index the answer of the brute-force cg_nearest_neighbor, ties to the smaller index, whatever the cell.  `cKDTree` is the
alias a port of the reference uses: `from catgrasp_amd.neighbors import cKDTree` (k = 1, Euclidean, exact: all the reference
calls)."""
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


    def nearest(self, query, debug=False):
        """Per query point the closest indexed point, unbounded and exact (cg_grid_nearest) -> (index (M) int32, d^2 (M) float64); exact
        ties go to the smaller index.  Without an indexed point: (-1, +inf).  With debug=True also rounds (M) int32: the number of box
        rounds the query took, negated where the linear pass finished it."""
        q, m, order = self._queries(query)
        idx = torch.full((m,), -1, dtype=torch.int32, device=self.device)
        d2 = torch.full((m,), math.inf, dtype=torch.float64, device=self.device)
        rounds = torch.zeros((m,), dtype=torch.int32, device=self.device) if debug else None
        if order is not None:
            with torch.cuda.device(self.device):
                _status(L.lib().cg_grid_nearest(*self._grid(), _p(q), int(q.dtype == torch.float64), _p(order), m, _p(idx), _p(d2), _p(rounds),
                                                _stream()), 'cg_grid_nearest')
        return (idx, d2, rounds) if debug else (idx, d2)

    def ball_point(self, query, radius):
        """Per query point the indexed points within `radius` (cg_grid_count_within, cg_grid_ball_fill) -> (offsets (M + 1) int64,
        indices int32): the neighbours of query i are indices[offsets[i]:offsets[i + 1]], in ascending original index."""
        radius = self._radius(radius)
        q, m, order = self._queries(query)
        offsets = torch.zeros((m + 1,), dtype=torch.int64, device=self.device)
        if order is None:
            return offsets, torch.empty((0,), dtype=torch.int32, device=self.device)
        count = torch.empty((m,), dtype=torch.int32, device=self.device)
        grid, f64 = self._grid(), int(q.dtype == torch.float64)
        with torch.cuda.device(self.device):
            _status(L.lib().cg_grid_count_within(*grid, _p(q), f64, _p(order), m, radius, _p(count), _stream()), 'cg_grid_count_within')
            offsets[1:] = torch.cumsum(count, 0, dtype=torch.int64)
            total = int(offsets[-1])
            indices = torch.empty((total,), dtype=torch.int32, device=self.device)
            _status(L.lib().cg_grid_ball_fill(*grid, _p(q), f64, _p(order), m, radius, _p(offsets), total, _p(indices), _stream()),
                    'cg_grid_ball_fill')
        # the kernel fills a segment in scan order: sort by (query, index), one key each (m n < 2^62)
        owner = torch.repeat_interleave(torch.arange(m, device=self.device), count.long(), output_size=total)
        key = torch.sort(owner * self.n + indices.long()).values
        return offsets, (key - owner * self.n).to(torch.int32)


def default_cell(lo, hi, n):
    """The cell cKDTree indexes a cloud with when none is given: the pitch at which an occupied cell holds about 4 points, for a cloud
    that fills its bounding box (cbrt(4 V / n)), one that is a surface in it (sqrt(4 A / n), A the product of the two largest
    extents) or a line (4 L / n), whichever is largest; 1 for a cloud without extent.  It decides speed only: no result depends on it."""
    e = sorted((float(h) - float(l) for l, h in zip(lo, hi)), reverse=True)
    n = max(int(n), 1)
    cell = max((4.0 * e[0] * e[1] * e[2] / n) ** (1.0 / 3.0), math.sqrt(4.0 * e[0] * e[1] / n), 4.0 * e[0] / n)
    return cell if math.isfinite(cell) and cell * cell >= sys.float_info.min else 1.0


class cKDTree:
    """scipy.spatial.cKDTree at the calls the reference makes, on the grid index: `cKDTree(data).query(x)`,
    `.query(x, distance_upper_bound=r)`, `.query_ball_point(x, r[, return_length=True])`; `.n`, `.m` (3) and `.data` as scipy has them.
    data: (N, 3) float32 or float64, array or tensor.  cell: the pitch of the index, default_cell() of the data unless given; it decides
    speed only.  Exact: k = 1, the Euclidean metric, eps = 0 -- the reference asks nothing else, and anything else raises
    NotImplementedError.  Exact ties go to the smaller index (scipy does not state its rule)."""

    m = 3

    def __init__(self, data, cell=None, device=None):
        pts = _cloud(data, 'data')
        self.n = int(pts.shape[0])
        self.data = pts.cpu().numpy()
        if cell is None:
            cell = default_cell(self.data.min(axis=0), self.data.max(axis=0), self.n) if self.n else 1.0
        self.index = GridIndex(pts, cell, device=device)
        self.device = self.index.device
        self._wider = {}                                              # radius -> the GridIndex with that cell, for query_ball_point beyond the cell

    def _points(self, x, what):
        """-> ((M, 3) cloud, whether x was one point)"""
        if not torch.is_tensor(x):
            x = np.asarray(x)
            if x.dtype not in (np.float32, np.float64):
                x = x.astype(np.float64)
        single = x.ndim == 1
        return _cloud(x.reshape(1, -1) if single else x, what), single

    def query(self, x, k=1, eps=0, p=2, distance_upper_bound=math.inf, return_tensor=False):
        """-> (distances float64, indices int64) of the nearest point of data per row of x, numpy arrays unless return_tensor; scalars
        for a single point (3,).  Without a point within distance_upper_bound (d <= bound counts as within): (inf, n)."""
        if k != 1 or p != 2 or eps != 0:
            raise NotImplementedError(f'cKDTree.query: only k=1, p=2, eps=0 are built (the reference uses nothing else); got k={k!r}, p={p!r}, '
                                      f'eps={eps!r}')
        bound = float(distance_upper_bound)
        if not bound >= 0:
            raise ValueError(f'distance_upper_bound must be >= 0, got {distance_upper_bound!r}')
        q, single = self._points(x, 'x')
        if bound <= self.index.cell and bound * bound >= sys.float_info.min:
            idx, d2 = self.index.nearest_within(q, bound)
        else:
            idx, d2 = self.index.nearest(q)
            if math.isfinite(bound):
                miss = ~(d2 <= bound * bound)
                idx, d2 = idx.masked_fill(miss, -1), d2.masked_fill(miss, math.inf)
        idx = idx.long()
        dist, idx = torch.sqrt(d2), torch.where(idx < 0, self.n, idx)
        if single:
            dist, idx = dist[0], idx[0]
        if return_tensor:
            return dist, idx
        return (float(dist), int(idx)) if single else (dist.cpu().numpy(), idx.cpu().numpy())

    def query_ball_point(self, x, r, p=2, eps=0, return_length=False):
        """-> per row of x the indices of the points of data within r (d <= r), ascending: an object array of lists, or the lengths
        with return_length; for a single point (3,) one list or one number.  A radius above the index's cell builds a second index with
        cell = r, which is kept for the next call."""
        if p != 2 or eps != 0:
            raise NotImplementedError(f'cKDTree.query_ball_point: only p=2, eps=0 are built (the reference uses nothing else); got p={p!r}, '
                                      f'eps={eps!r}')
        r = _positive(r, 'r')
        q, single = self._points(x, 'x')
        index = self.index
        if r > index.cell:
            index = self._wider.get(r)
            if index is None:
                index = self._wider[r] = GridIndex(self.data, r, device=self.device)
        if return_length:
            count = index.count_within(q, r).cpu().numpy().astype(np.intp)
            return int(count[0]) if single else count
        offsets, indices = index.ball_point(q, r)
        offsets, indices = offsets.cpu().tolist(), indices.cpu().tolist()
        out = np.empty((len(offsets) - 1,), dtype=object)
        for i in range(len(out)):
            out[i] = indices[offsets[i]:offsets[i + 1]]
        return out[0] if single else out


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
