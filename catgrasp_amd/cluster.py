"""Drop-in for `sklearn.cluster.MeanShift` as the reference calls it (predicter.py:332), on the device:

    from catgrasp_amd.cluster import MeanShift
    labels = MeanShift(bandwidth=bandwidth, cluster_all=True, n_jobs=-1, seeds=None).fit_predict(xyz_shifted)

The seed climb and the ordered merge are HIP kernels (csrc/meanshift.hip), the (count, center) ordering between them is a chain of
stable torch sorts on the device, the labels are cg_nearest_neighbor's.  All arithmetic is float64 on the exact coordinates of `X`."""
import numpy as np
import torch

from . import _lib as L
from ._lib import _p, _stream, check

ROUTES = {'auto': 0, 'lds': 1, 'streamed': 2}


def _device_points(X, device, what):
    """(n,3) numpy array or tensor, float32 or float64 -> contiguous device tensor of the same dtype; refuses non-finite values."""
    t = X if torch.is_tensor(X) else torch.from_numpy(np.ascontiguousarray(X))
    if t.dim() != 2 or t.shape[1] != 3 or t.shape[0] == 0:
        raise ValueError(f'{what} must be a non-empty (n, 3) array, got shape {tuple(t.shape)}')
    if t.dtype not in (torch.float32, torch.float64):
        t = t.to(torch.float64)
    t = t.to(device).contiguous()
    if not bool(torch.isfinite(t).all()):
        raise ValueError(f'{what} contains NaN or infinity')
    return t


def climb(pts, seeds, bandwidth, max_iter=300, route='auto'):
    """cg_meanshift_climb: pts (n,3) f32|f64 device tensor, seeds (m,3) f64 device tensor -> means (m,3) f64, counts (m) i32,
    iters (m) i32.  `route` ('auto', 'lds', 'streamed') exists for tests: the routes give identical bits."""
    L.require_cuda(pts, seeds)
    assert pts.dtype in (torch.float32, torch.float64) and pts.is_contiguous() and seeds.dtype == torch.float64 and seeds.is_contiguous()
    m = seeds.shape[0]
    means = torch.empty((m, 3), dtype=torch.float64, device=pts.device)
    counts = torch.empty((m,), dtype=torch.int32, device=pts.device)
    iters = torch.empty((m,), dtype=torch.int32, device=pts.device)
    check(L.lib().cg_meanshift_climb(_p(pts), int(pts.dtype == torch.float64), pts.shape[0], _p(seeds), m, float(bandwidth), int(max_iter),
                                     ROUTES[route], _p(means), _p(counts), _p(iters), _stream()), 'cg_meanshift_climb')
    return means, counts, iters


def sort_centers(means, counts):
    """scikit-learn's order of the non-empty seeds' centers: by (count, (x, y, z)) descending -- four stable sorts, least significant
    key first.  -> the sorted centers (m,3) f64."""
    alive = counts > 0
    c, k = means[alive], counts[alive]
    order = torch.arange(c.shape[0], device=c.device)
    for key in (c[:, 2], c[:, 1], c[:, 0], k):
        order = order[torch.sort(key[order], stable=True, descending=True).indices]
    return c[order].contiguous()


def merge(sorted_centers, bandwidth):
    """cg_meanshift_merge -> the kept centers, in order."""
    keep = torch.empty((sorted_centers.shape[0],), dtype=torch.uint8, device=sorted_centers.device)
    check(L.lib().cg_meanshift_merge(_p(sorted_centers), sorted_centers.shape[0], float(bandwidth), _p(keep), _stream()), 'cg_meanshift_merge')
    return sorted_centers[keep.bool()].contiguous()


def nearest_center(pts, centers):
    """Index of the nearest center per point (float64, first minimum) and its distance."""
    q = pts.to(torch.float64).contiguous()
    idx = torch.empty((q.shape[0],), dtype=torch.int32, device=q.device)
    check(L.lib().cg_nearest_neighbor(_p(q), q.shape[0], _p(centers), centers.shape[0], _p(idx), _stream()), 'cg_nearest_neighbor')
    idx = idx.long()
    return idx, torch.linalg.vector_norm(q - centers[idx], dim=1)


class MeanShift:
    """sklearn.cluster.MeanShift with a given bandwidth and a flat kernel.  `n_jobs` is accepted and ignored; `bandwidth=None`
    (estimate_bandwidth) and `bin_seeding=True` are not built: the reference uses neither.  `fit` needs a HIP device."""

    def __init__(self, bandwidth=None, seeds=None, bin_seeding=False, min_bin_freq=1, cluster_all=True, n_jobs=None, max_iter=300,
                 _route='auto'):
        if bandwidth is None:
            raise NotImplementedError('MeanShift(bandwidth=None): estimate_bandwidth is not built; pass the bandwidth')
        if bin_seeding:
            raise NotImplementedError('MeanShift(bin_seeding=True) is not built; seeds are all points or an explicit array')
        if not (np.isfinite(bandwidth) and bandwidth > 0):
            raise ValueError(f'bandwidth must be a positive finite number, got {bandwidth!r}')
        if int(max_iter) < 0:
            raise ValueError(f'max_iter must be >= 0, got {max_iter!r}')
        self.bandwidth, self.seeds, self.bin_seeding, self.min_bin_freq = float(bandwidth), seeds, bin_seeding, min_bin_freq
        self.cluster_all, self.n_jobs, self.max_iter, self._route = cluster_all, n_jobs, int(max_iter), _route

    def _device(self, X):
        if torch.is_tensor(X) and X.is_cuda:
            return X.device
        if not torch.cuda.is_available():
            raise L.CatgraspAmdError('catgrasp_amd.cluster needs a HIP device (no CPU fallback)')
        return torch.device('cuda', torch.cuda.current_device())

    def fit(self, X, y=None):
        dev = self._device(X)
        pts = _device_points(X, dev, 'X')
        seeds = pts.to(torch.float64) if self.seeds is None else _device_points(self.seeds, dev, 'seeds').to(torch.float64)
        means, counts, iters = climb(pts, seeds.contiguous(), self.bandwidth, self.max_iter, self._route)
        self.n_iter_ = int(iters.max())
        centers = sort_centers(means, counts)
        if centers.shape[0] == 0:
            raise ValueError('No point was within bandwidth=%f of any seed. Try a different seeding strategy '
                             'or increase the bandwidth.' % self.bandwidth)
        self._centers = merge(centers, self.bandwidth)
        labels, dist = nearest_center(pts, self._centers)
        if not self.cluster_all:
            labels = torch.where(dist <= self.bandwidth, labels, torch.full_like(labels, -1))
        self._labels = labels
        self.cluster_centers_, self.labels_ = self._centers.cpu().numpy(), labels.cpu().numpy()
        return self

    def fit_predict(self, X, y=None):
        return self.fit(X).labels_

    def predict(self, X):
        if not hasattr(self, '_centers'):
            raise L.CatgraspAmdError('MeanShift.predict before fit')
        pts = _device_points(X, self._centers.device, 'X')
        return nearest_center(pts, self._centers)[0].cpu().numpy()
