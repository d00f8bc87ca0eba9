"""GPU tests of the grid index (csrc/grid_index.hip, catgrasp_amd/neighbors.py).

The normals of an unorganized cloud are held three ways:
  * on the used points of a depth image, in row-major order, they are THE SAME BITS as cg_organized_normals' -- two independent search
    structures (pixel window, cell lattice), one result;
  * on any other point list, to the bars of tests/test_scene_gpu.py against scene_ref.organized_normals of that list: neighbour count
    and largest neighbour d2 bit-equal, the default normal bit-equal,
        n^T C n - lambda_1 <= 1e-11 lambda_3,   | |n| (1 + 1e-10) - 1 | <= 1e-12,   view . n >= 0,   | n - n_ref | <= 1e-9
    (the reasons for these figures are in that module's docstring; tests/test_neighbors_ref_cpu.py asserts that every cloud here has
    the gap, the distance from ties and the |view . n| they need);
  * across cell sizes, bit for bit.
The radius queries are exact against the float64 brute force of tests/neighbors_ref.py: index, d2 bits and count."""
import numpy as np
import pytest
import torch

import neighbors_ref as N
import scene_ref as R
from catgrasp_amd import _lib as L
from catgrasp_amd import neighbors, scene

pytestmark = pytest.mark.gpu
DEFAULT = np.array([0.0, 0.0, -1.0]) / (1 + 1e-10)                          # (0,0,1), oriented towards a camera at the origin


def _grid_normals(P, dev, radius, max_nn, cell=None):
    n, c, d = neighbors.GridIndex(torch.tensor(P, device=dev), radius if cell is None else cell).estimate_normals(
        radius, max_nn, debug=True)
    assert n.dtype == torch.float64 and c.dtype == torch.int32 and d.dtype == torch.float64 and n.is_cuda
    return n, c, d


def _check_against(ref, normals, count, d2max, max_nn, ties=False):
    """The bars of the module docstring on every point; with `ties` the cloud has exact ties on purpose and only the scene's gap is asked."""
    ok = ref['count'] >= 3
    lam = ref['lam']
    if max_nn >= 3:
        assert ties or int(ref['tie'].sum()) == 0
        assert ((lam[ok, 1] - lam[ok, 0]) / lam[ok, 2]).min() >= 1e-3
    assert np.abs((ref['view'] * ref['normals']).sum(axis=1)).min() >= 1e-6
    assert np.array_equal(count, ref['count']) and np.array_equal(d2max.view(np.uint64), ref['d2max'].view(np.uint64))
    assert np.array_equal(normals[~ok], ref['normals'][~ok])
    rayleigh = np.einsum('ni,nij,nj->n', normals, ref['C'], normals) * (1 + 1e-10) ** 2
    print('max (n^T C n - l1) / l3', ((rayleigh - lam[:, 0])[ok] / lam[ok, 2]).max() if ok.any() else 0.0,
          'max |n - n_ref|', np.abs(normals - ref['normals']).max())
    assert ((rayleigh - lam[:, 0])[ok] <= 1e-11 * lam[ok, 2]).all()
    assert (np.abs(np.linalg.norm(normals, axis=1) * (1 + 1e-10) - 1) <= 1e-12).all()
    assert ((ref['view'] * normals).sum(axis=1) >= 0).all()
    assert (np.abs(normals - ref['normals']) <= 1e-9).all()


@pytest.mark.parametrize('radius,max_nn', [(0.002, 30), (0.003, 30), (0.002, 1), (0.002, 2), (0.003, 64)])
@pytest.mark.parametrize('name', ['A', 'B'])
def test_on_a_depth_image_the_grid_gives_the_bits_of_the_organized_kernel(cuda_device, name, radius, max_nn):
    depth, bg, K = (*R.scene_a(), R.K_A) if name == 'A' else (R.scene_b(), None, R.K_B)
    xyz, valid = R.depth2xyzmap(depth, K)
    use = valid if bg is None else valid & ~bg
    d_xyz, d_use = torch.from_numpy(xyz).to(cuda_device), torch.from_numpy(use).to(cuda_device)
    want = scene.estimate_normals_organized(d_xyz, d_use, K, radius=radius, max_nn=max_nn, debug=True)
    P = d_xyz[d_use]
    assert np.array_equal(P.cpu().numpy(), N.cloud(name)) and len(P) == (6551 if name == 'A' else 1600)
    got = neighbors.estimate_normals(P, radius=radius, max_nn=max_nn, return_tensor=True, debug=True)
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and torch.equal(g, w[d_use])
    if max_nn == 64:
        assert int(got[1].max()) == 64 and int((got[1] > 30).sum()) > len(P) // 2         # the long lists are exercised
    if name == 'B' and (radius, max_nn) == (0.002, 30):
        assert int(N.normals_ref('B')['tie'].sum()) == 1450                                # the tie rule decides here


def test_permuted_scene_a_meets_the_bars_of_the_organized_tests(cuda_device):
    ref = N.normals_ref('A_perm')
    n, c, d = (t.cpu().numpy() for t in _grid_normals(N.cloud('A_perm'), cuda_device, 0.002, 30))
    _check_against(ref, n, c, d, 30)
    lone = np.nonzero(ref['count'] == 1)[0]
    assert len(lone) == 1 and np.array_equal(n[lone[0]], DEFAULT)
    # the same points in another order: the same neighbour sets, so count and d2max are those of the row-major cloud, permuted
    perm = np.random.default_rng(11).permutation(len(c))
    row_major = N.normals_ref('A')
    assert np.array_equal(c, row_major['count'][perm]) and np.array_equal(d, row_major['d2max'][perm])


def test_permuted_scene_b_ties_go_to_the_smaller_point_index(cuda_device):
    lo, hi = N.normals_ref('B_perm'), N.normals_ref('B_perm', prefer='high')
    # CPU side: 1,450 exact ties at the 30th place, and the opposite rule misses the componentwise bar at every one of them
    assert int(lo['tie'].sum()) == 1450
    assert int((np.abs(hi['normals'] - lo['normals']).max(axis=1) > 1e-9).sum()) == 1450
    n, c, d = (t.cpu().numpy() for t in _grid_normals(N.cloud('B_perm'), cuda_device, 0.002, 30))
    _check_against(lo, n, c, d, 30, ties=True)


@pytest.mark.parametrize('radius,max_nn', [(0.002, 30), (0.003, 30), (0.002, 8)])
def test_a_cloud_that_never_was_an_image(cuda_device, radius, max_nn):
    ref = N.normals_ref('sheet', radius, max_nn)
    assert len(ref['count']) == 7502 and int((ref['count'] < 3).sum()) == 2
    n, c, d = (t.cpu().numpy() for t in _grid_normals(N.cloud('sheet'), cuda_device, radius, max_nn))
    _check_against(ref, n, c, d, max_nn)


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_millimetre_lattice_pairs_at_the_bound_are_counted_as_brute_force_counts_them(cuda_device, dtype):
    P = N.mm_lattice(dtype)
    r = 0.002
    want = N.count_within(P, P, r)
    assert 30 < want.max() < 33 and len(np.unique(want)) > 10               # rounding alone decides the pairs two steps apart
    index = neighbors.GridIndex(torch.from_numpy(P).to(cuda_device), r)     # cell == radius
    assert np.array_equal(index.count_within(torch.from_numpy(P).to(cuda_device), r).cpu().numpy(), want)
    ref = R.organized_normals(P, r, 30)
    n, c, d = (t.cpu().numpy() for t in index.estimate_normals(r, 30, debug=True))
    assert np.array_equal(c, ref['count']) and np.array_equal(c, np.minimum(want, 30)) and np.array_equal(d.view(np.uint64), ref['d2max'].view(np.uint64))
    idx, d2 = index.nearest_within(P, r)
    assert np.array_equal(idx.cpu().numpy(), np.arange(len(P))) and not d2.any()


def test_power_of_two_lattice_takes_d2_equal_to_r2_and_breaks_ties_by_index(cuda_device):
    P = N.pow2_lattice()
    r = 2.0 ** -9
    want = N.count_within(P, P, r)
    assert want.max() == 33 and int((N.d2_matrix(P, P) == r * r).sum()) == 3402
    ref = R.organized_normals(P, r, 30)
    assert int(ref['tie'].sum()) == 335
    index = neighbors.GridIndex(P, r, device=cuda_device)
    assert np.array_equal(index.count_within(P, r).cpu().numpy(), want)
    n, c, d = (t.cpu().numpy() for t in index.estimate_normals(r, 30, debug=True))
    assert np.array_equal(c, ref['count']) and np.array_equal(d.view(np.uint64), ref['d2max'].view(np.uint64))
    # the covariances are isotropic, so only length and orientation are asked of the normals
    assert (np.abs(np.linalg.norm(n, axis=1) * (1 + 1e-10) - 1) <= 1e-12).all() and ((ref['view'] * n).sum(axis=1) >= 0).all()
    # with max_nn = 33 nothing is tied away, and the uncapped count comes out
    assert np.array_equal(index.estimate_normals(r, 33, debug=True)[1].cpu().numpy(), want)


def _queries(P):
    """The cloud's own points, points outside its box by less and by more than either radius, and one 10 m away."""
    lo, hi = P.min(axis=0).astype(np.float64), P.max(axis=0).astype(np.float64)
    sheet = P[np.abs(P[:, 2] - 0.6) < 0.01].astype(np.float64)
    edge = sheet[np.argmin(sheet[:, 0])]                                    # the sheet's point of smallest x
    extra = [[edge[0] - 0.001, edge[1], edge[2]], [edge[0] - 0.004, edge[1], edge[2]], [edge[0] - 0.0051, edge[1], edge[2]],
             [lo[0] - 0.0015, 0.1, 0.4], [lo[0] - 0.02, 0.1, 0.4], [0.2, hi[1] + 0.0019, 0.9], [0.2, 0.2, hi[2] + 0.0049], [0.2, 0.2, hi[2] + 0.0051],
             [10.0, 0.0, 0.6], [0.0, -10.0, 0.6], [0.0, 0.0, -9.4], [1e150, -1e150, 1e150]]
    return np.concatenate((P.astype(np.float64), np.array(extra)))


@pytest.mark.parametrize('radius', [0.002, 0.005])
def test_radius_queries_equal_brute_force_exactly(cuda_device, radius):
    P = N.cloud('sheet')
    Q = _queries(P)
    want_i, want_d = N.nearest_within(P, Q, radius)
    want_c = N.count_within(P, Q, radius)
    assert 0 < int((want_i[len(P):] >= 0).sum()) < len(Q) - len(P) and want_c.max() > 30
    index = neighbors.GridIndex(torch.tensor(P, device=cuda_device), radius)
    for q in (Q, torch.from_numpy(Q).to(cuda_device), Q[::-1].copy()):
        flip = q is not Q and not torch.is_tensor(q)
        idx, d2 = index.nearest_within(q, radius)
        cnt = index.count_within(q, radius)
        assert idx.dtype == torch.int32 and d2.dtype == torch.float64 and cnt.dtype == torch.int32
        idx, d2, cnt = (t.cpu().numpy()[::-1] if flip else t.cpu().numpy() for t in (idx, d2, cnt))
        assert np.array_equal(idx, want_i) and np.array_equal(d2.view(np.uint64), want_d.view(np.uint64)) and np.array_equal(cnt, want_c)
    # float32 queries are widened exactly
    Q32 = Q[:-1].astype(np.float32)
    idx, d2 = index.nearest_within(Q32, radius)
    want_i, want_d = N.nearest_within(P, Q32, radius)
    assert np.array_equal(idx.cpu().numpy(), want_i) and np.array_equal(d2.cpu().numpy().view(np.uint64), want_d.view(np.uint64))
    assert np.array_equal(index.count_within(Q32, radius).cpu().numpy(), N.count_within(P, Q32, radius))


def test_duplicated_points_give_the_smaller_index_and_count_twice(cuda_device):
    P = N.cloud('sheet').copy()
    P[4000] = P[7]
    index = neighbors.GridIndex(P, 0.002, device=cuda_device)
    idx, d2 = index.nearest_within(P[[7, 4000, 8]], 0.002)
    assert idx.tolist() == [7, 7, 8] and d2.tolist() == [0.0, 0.0, 0.0]
    assert np.array_equal(index.count_within(P, 0.002).cpu().numpy(), N.count_within(P, P, 0.002))
    ref = R.organized_normals(P, 0.002, 30)
    n, c, d = (t.cpu().numpy() for t in index.estimate_normals(0.002, 30, debug=True))
    assert np.array_equal(c, ref['count']) and np.array_equal(d.view(np.uint64), ref['d2max'].view(np.uint64))
    assert np.array_equal(n[7], n[4000])                                    # the same candidates, the same order of accumulation


def test_cloud_a_minus_cloud_b_keeps_what_brute_force_keeps(cuda_device):
    P = N.cloud('sheet')
    sheet = P[np.abs(P[:, 2] - 0.6) < 0.01]
    patch = sheet[np.linalg.norm(sheet[:, :2] - [0.01, -0.005], axis=1) < 0.008]
    want_pts, want_ids = N.cloudA_minus_cloudB(sheet, patch, 0.005)
    assert 0 < len(want_ids) < len(sheet) - len(patch)
    pts, ids = neighbors.cloudA_minus_cloudB(sheet, patch, 0.005)
    assert isinstance(pts, np.ndarray) and np.array_equal(ids, want_ids) and np.array_equal(pts, want_pts) and (np.diff(ids) > 0).all()
    t_pts, t_ids = neighbors.cloudA_minus_cloudB(torch.from_numpy(sheet).to(cuda_device), torch.from_numpy(patch), 0.005)
    assert t_pts.is_cuda and np.array_equal(t_ids.cpu().numpy(), want_ids) and np.array_equal(t_pts.cpu().numpy(), want_pts)
    # nothing to subtract, and everything
    assert np.array_equal(neighbors.cloudA_minus_cloudB(sheet, patch[:0], 0.005)[1], np.arange(len(sheet)))
    assert len(neighbors.cloudA_minus_cloudB(sheet, sheet, 0.005)[1]) == 0


def test_the_cell_size_never_shows(cuda_device):
    P = torch.tensor(N.cloud('sheet'), device=cuda_device)
    Q = torch.from_numpy(_queries(N.cloud('sheet'))).to(cuda_device)
    radius = 0.002
    outs = []
    for cell in (radius, 1.5 * radius, 4 * radius):
        index = neighbors.GridIndex(P, cell)
        outs.append((*index.estimate_normals(radius, 30, debug=True), *index.nearest_within(Q, radius), index.count_within(Q, radius)))
    for other in outs[1:]:
        for a, b in zip(outs[0], other):
            assert torch.equal(a, b)
    assert torch.equal(neighbors.GridIndex(P, radius).estimate_normals(), outs[0][0])             # radius defaults to the cell
    index = neighbors.GridIndex(P, radius)
    for call in (lambda: index.estimate_normals(radius * 1.0001), lambda: index.nearest_within(Q, 0.005), lambda: index.count_within(Q, 0.0021)):
        with pytest.raises(ValueError, match='exceeds'):
            call()


def test_f64_input_gives_the_bits_of_the_f32_run(cuda_device):
    P = N.cloud('sheet')
    a = _grid_normals(P, cuda_device, 0.002, 30)
    b = _grid_normals(P.astype(np.float64), cuda_device, 0.002, 30)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    # and values that are no float32 are not rounded to one: the neighbour sets move
    shifted = P.astype(np.float64) * (1 + 2.0 ** -30)
    ref = R.organized_normals(shifted, 0.002, 30)
    n, c, d = (t.cpu().numpy() for t in _grid_normals(shifted, cuda_device, 0.002, 30))
    assert np.array_equal(c, ref['count']) and np.array_equal(d.view(np.uint64), ref['d2max'].view(np.uint64))
    assert not np.array_equal(d, a[2].cpu().numpy())


def test_degenerate_inputs(cuda_device, monkeypatch):
    one = np.array([[0.01, -0.02, 0.5]], np.float32)
    n, c, d = _grid_normals(one, cuda_device, 0.002, 30)
    assert c.tolist() == [1] and d.tolist() == [0.0] and np.array_equal(n.cpu().numpy()[0], DEFAULT)
    same = np.tile(one, (200, 1))
    n, c, d = (t.cpu().numpy() for t in _grid_normals(same, cuda_device, 0.002, 30))
    assert (c == 30).all() and not d.any() and np.isfinite(n).all()
    assert (np.abs(np.linalg.norm(n, axis=1) * (1 + 1e-10) - 1) <= 1e-12).all() and ((-same.astype(np.float64)) * n).sum(axis=1).min() >= 0
    index = neighbors.GridIndex(same, 0.002, device=cuda_device)
    assert index.count_within(one, 0.002).tolist() == [200] and index.nearest_within(one, 0.002)[0].tolist() == [0]
    # empty cloud, empty queries: empty (or "nothing found") outputs, and no launch -- cg_* would refuse n = 0
    calls = []
    real = L.lib()

    class Spy:
        def __getattr__(self, name):
            calls.append(name)
            return getattr(real, name)
    monkeypatch.setattr(L, 'lib', lambda: Spy())
    empty = neighbors.GridIndex(np.zeros((0, 3), np.float32), 0.002, device=cuda_device)
    n, c, d = empty.estimate_normals(debug=True)
    assert tuple(n.shape) == (0, 3) and n.dtype == torch.float64 and c.numel() == 0 and d.numel() == 0
    idx, d2 = empty.nearest_within(one, 0.002)
    assert idx.tolist() == [-1] and d2.tolist() == [float('inf')] and empty.count_within(one, 0.002).tolist() == [0]
    assert neighbors.estimate_normals(np.zeros((0, 3))).shape == (0, 3)
    assert calls == []
    idx, d2 = index.nearest_within(np.zeros((0, 3)), 0.002)
    assert idx.numel() == 0 and d2.numel() == 0 and index.count_within(torch.zeros((0, 3), device=cuda_device), 0.002).numel() == 0
    assert calls == []
    monkeypatch.undo()
    # refusals
    bad = N.cloud('sheet').copy()
    for v in (np.nan, np.inf):
        bad[100, 2] = v
        with pytest.raises(ValueError, match='NaN or infinity'):
            neighbors.GridIndex(bad, 0.002, device=cuda_device)
        with pytest.raises(ValueError, match='NaN or infinity'):
            index.nearest_within(bad, 0.002)
    with pytest.raises(NotImplementedError, match='64'):
        index.estimate_normals(0.002, 65)
    with pytest.raises(ValueError, match='max_nn'):
        index.estimate_normals(0.002, 0)
    assert index.estimate_normals(0.002, 64, debug=True)[1].tolist() == [64] * 200
    with pytest.raises(L.CatgraspAmdError, match='HIP device'):
        neighbors.GridIndex(torch.from_numpy(one), 0.002, device='cpu')
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    with pytest.raises(L.CatgraspAmdError, match='HIP device'):
        neighbors.GridIndex(torch.from_numpy(one), 0.002)
    # a lattice too fine for 62 bits
    with pytest.raises(ValueError, match='62 bits'):
        neighbors.GridIndex(np.array([[0.0, 0.0, 0.0], [1.0, 1.0, 1.0]]), 1e-7, device=cuda_device)


def test_scene_from_depth_adds_the_normals_of_the_down_sampled_scene(cuda_device):
    depth, bg = R.scene_a()
    plain = scene.scene_from_depth(depth, R.K_A, bg_mask=bg)
    out = scene.scene_from_depth(depth, R.K_A, bg_mask=bg, scene_normal_radius=0.003)
    assert sorted(plain) == ['data', 'scene_pts'] and sorted(out) == ['data', 'scene_normals', 'scene_pts']
    assert sorted(plain['data']) == sorted(out['data']) == ['cloud_normal', 'cloud_xyz']
    for k in plain['data']:
        assert np.array_equal(plain['data'][k], out['data'][k])
    assert np.array_equal(plain['scene_pts'], out['scene_pts'])
    want = neighbors.estimate_normals(out['scene_pts'], 0.003)
    assert isinstance(out['scene_normals'], np.ndarray) and out['scene_normals'].dtype == np.float64
    assert out['scene_normals'].shape == out['scene_pts'].shape and np.array_equal(out['scene_normals'], want)
    # the down-sampled cloud is no image: its normals are held to the restatement over its point list
    ref = R.organized_normals(out['scene_pts'], 0.003, 30)
    assert (np.abs(np.linalg.norm(want, axis=1) * (1 + 1e-10) - 1) <= 1e-12).all() and ((ref['view'] * want).sum(axis=1) >= 0).all()
    settled = (ref['count'] >= 3) & ~ref['tie']
    settled[settled] = (ref['lam'][settled, 1] - ref['lam'][settled, 0]) / ref['lam'][settled, 2] >= 1e-3
    assert int(settled.sum()) > len(settled) // 2 and (np.abs(want - ref['normals'])[settled] <= 1e-9).all()
    tensors = scene.scene_from_depth(depth, R.K_A, bg_mask=bg, scene_normal_radius=0.003, return_tensor=True)
    assert tensors['scene_normals'].is_cuda and np.array_equal(tensors['scene_normals'].cpu().numpy(), want)
