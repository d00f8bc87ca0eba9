"""cg_occupancy_set_bits and cg_occupancy_grid_rays (csrc/occupancy.hip) on the constructed rays, bitmaps and clouds of
tests/occupancy_cases.py, which tests/test_occupancy_cases_cpu.py certifies from the C oracle alone.  The kernels are called through the
C entry points with hand-built key boxes; a ray case is a 1 x 1 x 1 lattice whose origin is the query.  Every comparison is equality:
keep bytes against the constructed flag AND the oracle's (cast_ray + the restated keep rule), lattice bits, bitmap words; outputs are
sentinel-filled with guard elements behind them.

Branch of csrc/occupancy.hip                                 -> test that pins it
  occupancy_rays_kernel: dim choice on tMax ties (`<`)         test_ray_cases[tie-*] (all eight octants, face diagonals)
                         step 0 on one / two / three axes      test_ray_cases[axis*, tie-face*, zero-query-*]
                         origin leaf occupied                  test_ray_cases[origin-leaf-*, zero-query-occupied-origin]
                         keep: dist <= dist_query              test_ray_cases[keep-z*, origin-leaf-q-at-centre (equality)]
                         range test before occupancy test      test_ray_cases[range-*] (the floats just below / above sqrt(dsq))
                         walk ends at key +-32768              test_walk_ends_at_the_key_border
                         lattice coordinates, tail block       test_lattice_bits_tail_and_guards[7x5x11, 1x1x1]
  occupied(): box offsets, out-of-box index -1 and d           test_out_of_box_lookups_are_free
  set_bits_kernel: bit index, word boundaries, duplicates      test_set_bits_words
  entry points: n = 0, resolution <= 0, n_keys = 0             test_lattice_bits_tail_and_guards, test_set_bits_words
  my_cpp.makeOccupancyGridFromCloudScan                        test_wrapper_on_hand_clouds[*]

Measured on an MI355X: no test takes more than 0.3 s (the wrapper clouds); a walk to the key border takes 10 ms on an axis, 30 ms on the
diagonal (test_walk_ends_at_the_key_border prints them as TIME)."""
import time

import numpy as np
import pytest
import torch

import occupancy_cases as oc
from oracle import collision_oracle as co

pytestmark = pytest.mark.gpu
GUARD = 8
F_SENTINEL, K_SENTINEL, W_SENTINEL = -123.5, 0xA5, 0x5A5A5A5A


def _d(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _keys4(keys):
    k = np.zeros((len(keys), 4), dtype=np.int16)
    if len(keys):
        k[:, :3] = np.asarray(keys, dtype=np.int16).reshape(-1, 3)
    return k


def _set_bits(dev, keys, offset, dims, prefill=0, n_keys=None):
    """-> status, the bitmap words after the call (guard words checked)"""
    from catgrasp_amd import _lib as L
    if min(dims) > 0:
        for key in keys:              # every key inside the box (asserted): the kernel does not check
            oc.bit_index(key, offset, dims)
    nw = (dims[0] * dims[1] * dims[2] + 31) // 32
    words = np.full(nw + GUARD, W_SENTINEL, dtype=np.uint32); words[:nw] = prefill
    bits = _d(words.view(np.int32), dev)
    d_keys = _d(_keys4(keys if len(keys) else [(0, 0, 0)]), dev)
    st = L.lib().cg_occupancy_set_bits(L._p(d_keys), len(keys) if n_keys is None else n_keys, L._p(bits), *offset, *dims, L._stream())
    w = bits.cpu().numpy().view(np.uint32)
    assert (w[nw:] == W_SENTINEL).all(), 'guard words written'
    return st, w[:nw], bits


def _rays(dev, bits, offset, dims, origin, res, n, max_range, wait=None):
    """-> status, lattice (total,3) float32, keep (total) uint8; guards checked"""
    from catgrasp_amd import _lib as L
    total = max(n[0], 0) * max(n[1], 0) * max(n[2], 0)
    lattice = torch.full((total + GUARD, 3), F_SENTINEL, dtype=torch.float32, device=dev)
    keep = torch.full((total + GUARD,), K_SENTINEL, dtype=torch.uint8, device=dev)
    st = L.lib().cg_occupancy_grid_rays(L._p(bits), *offset, *dims, float(origin[0]), float(origin[1]), float(origin[2]), float(res),
                                        n[0], n[1], n[2], float(max_range), L._p(lattice), L._p(keep), L._stream())
    if wait is not None:
        wait()
    la, k = lattice.cpu().numpy(), keep.cpu().numpy()
    assert (la[total:] == np.float32(F_SENTINEL)).all() and (k[total:] == K_SENTINEL).all(), 'guard elements written'
    return st, la[:total], k[:total]


def _box_of(leaves):
    """a key box around the leaves with a margin of one cell (an empty set: one cell far away)"""
    if not leaves:
        return (100, 100, 100), (1, 1, 1)
    k = np.asarray(leaves)
    lo, hi = k.min(axis=0) - 1, k.max(axis=0) + 1
    return tuple(int(v) for v in lo), tuple(int(v) for v in hi - lo + 1)


def _cast(dev, ray, res, offset=None, dims=None, wait=None):
    """one ray through the kernel -> keep byte"""
    if offset is None:
        offset, dims = _box_of(ray.leaves)
    st, w, bits = _set_bits(dev, ray.leaves, offset, dims)
    assert st == 0 and np.array_equal(w, oc.pack(ray.leaves, offset, dims))
    q = ray.query(res)
    st, la, k = _rays(dev, bits, offset, dims, q, res, (1, 1, 1), ray.range(res), wait)
    assert st == 0 and np.array_equal(la[0].view(np.uint32), q.view(np.uint32)) and k[0] in (0, 1), f'{ray}: lattice {la}, keep {k}'
    return int(k[0])


def _oracle_keep(ray, res):
    pts = oc.centres(ray.leaves, res) if ray.leaves else np.zeros((0, 3), dtype=np.float32)
    q = ray.query(res)
    hit, end = co.cast_ray(pts, np.float32(res), oc.direction(q), ray.range(res))
    return int(oc.keep_rule(q, hit, end))


@pytest.mark.parametrize('res', [oc.RES, oc.RES_MM], ids=['2^-10', '0.001f'])
def test_ray_cases(cuda_device, res):
    wrong = []
    for ray in oc.ray_cases(res):
        got, ref = _cast(cuda_device, ray, res), _oracle_keep(ray, res)
        assert ref == int(ray.keep), f'{ray}: the oracle ({ref}) is not the constructed outcome'
        if got != ref:
            wrong.append(f'{ray}: keep {got}, oracle {ref} (hit {ray.hit}, end {ray.end})')
    assert not wrong, f'{len(wrong)} rays differ:\n' + '\n'.join(wrong)


def test_walk_ends_at_the_key_border(cuda_device):
    """empty bitmap, no range: the walk must stop by itself at key +-32768 (about 1e5 steps for the diagonal: milliseconds).  The result is
    awaited with a deadline, so a walk that does not end fails here instead of stalling the run."""
    def wait():
        done = torch.cuda.Event(); done.record()
        t0 = time.perf_counter()
        while not done.query():
            if time.perf_counter() - t0 > 10.0:
                pytest.fail('the ray walk did not end within 10 s')
    for ray in oc.border_cases():
        t0 = time.perf_counter()
        assert _cast(cuda_device, ray, oc.RES, wait=wait) == 0 == _oracle_keep(ray, oc.RES), ray
        print(f'TIME {ray}: {1e3 * (time.perf_counter() - t0):.2f} ms')


def test_out_of_box_lookups_are_free(cuda_device):
    for ray in oc.box_face_cases():
        assert _cast(cuda_device, ray, oc.RES, ray.offset, oc.DIMS) == 0 == _oracle_keep(ray, oc.RES), ray
        # the same ray does report the cell once the box holds it
        ghost = oc.Ray(ray.name + '-ghost', 'in-box', [ray.ghost], ray.q, True, ray.ghost, True)
        assert _cast(cuda_device, ghost, oc.RES) == 1 == _oracle_keep(ghost, oc.RES), ghost


def test_set_bits_words(cuda_device):
    dev = cuda_device
    for key in oc.corners() + [oc.key_of_bit(i) for i in (31, 32, 63, 64, 95, 96)]:
        st, w, _ = _set_bits(dev, [key], oc.OFFSET, oc.DIMS)
        assert st == 0 and np.array_equal(w, oc.pack([key])), key
    keys = [oc.key_of_bit(i) for i in (0, 31, 32, 33, 63, 64, 104, 57)]
    st, w, _ = _set_bits(dev, keys, oc.OFFSET, oc.DIMS)
    assert st == 0 and np.array_equal(w, oc.pack(keys))
    st, w2, _ = _set_bits(dev, keys + keys[::-1] + keys[:3], oc.OFFSET, oc.DIMS)                  # duplicates change nothing
    assert st == 0 and np.array_equal(w2, w)
    st, w3, _ = _set_bits(dev, keys, oc.OFFSET, oc.DIMS, prefill=0x80000001)                      # bits are OR-ed in
    assert st == 0 and np.array_equal(w3, w | np.uint32(0x80000001))
    st, w4, _ = _set_bits(dev, [], oc.OFFSET, oc.DIMS, prefill=0x12345678)                        # n_keys = 0: OK, nothing written
    assert st == 0 and (w4 == 0x12345678).all()
    assert _set_bits(dev, keys, oc.OFFSET, (3, 0, 7), n_keys=1)[0] == -1 and _set_bits(dev, keys, oc.OFFSET, oc.DIMS, n_keys=-1)[0] == -1


@pytest.mark.parametrize('n', [oc.LATTICE_N, (1, 1, 1)], ids=['7x5x11', '1x1x1'])
@pytest.mark.parametrize('origin_leaf', [False, True], ids=['origin-free', 'origin-occupied'])
def test_lattice_bits_tail_and_guards(cuda_device, n, origin_leaf):
    from catgrasp_amd import _lib as L
    dev, res = cuda_device, oc.RES
    leaves = oc.LATTICE_LEAVES + ([(0, 0, 0)] if origin_leaf else [])
    offset, dims = _box_of(leaves)
    st, w, bits = _set_bits(dev, leaves, offset, dims)
    assert st == 0 and np.array_equal(w, oc.pack(leaves, offset, dims))
    origin = np.array(oc.LATTICE_ORIGIN, dtype=np.float32) * res
    max_range = np.float32(oc.RANGE * float(res))
    st, la, k = _rays(dev, bits, offset, dims, origin, res, n, max_range)
    ref_la = oc.lattice_points(origin, n, res)
    assert st == 0 and np.array_equal(la.view(np.uint32), ref_la.view(np.uint32))
    pts = oc.centres(leaves, res)
    ref_k = np.zeros(len(ref_la), dtype=np.uint8)
    for i, q in enumerate(ref_la):
        hit, end = co.cast_ray(pts, res, oc.direction(q), max_range)
        ref_k[i] = oc.keep_rule(q, hit, end)
    assert set(np.unique(k)) <= {0, 1} and np.array_equal(k, ref_k), f'{(k != ref_k).sum()} of {len(k)} lattice points differ'
    if len(k) > 1:
        if origin_leaf:           # every ray stops in the origin leaf, sqrt(0.75) res away: all kept but q = 0 itself
            assert ref_k.sum() == len(k) - 1 and not ref_k[(3 * 5 + 2) * 11 + 5]
        else:
            assert 20 < ref_k.sum() < len(k) - 20
        # an empty axis: OK and nothing written; a resolution that is not positive: refused before any launch
        for empty in ((0, 5, 11), (7, 0, 11), (7, 5, 0)):
            st, la, k = _rays(dev, bits, offset, dims, origin, res, empty, max_range)
            assert st == 0 and len(k) == 0
        for bad in (0.0, -1.0, float('nan')):
            lattice = torch.full((4, 3), F_SENTINEL, dtype=torch.float32, device=dev); keep = torch.full((4,), K_SENTINEL, dtype=torch.uint8, device=dev)
            st = L.lib().cg_occupancy_grid_rays(L._p(bits), *offset, *dims, 0.0, 0.0, 0.0, bad, 1, 1, 1, 0.0, L._p(lattice), L._p(keep), L._stream())
            assert st == -1 and (lattice.cpu().numpy() == np.float32(F_SENTINEL)).all() and (keep.cpu().numpy() == K_SENTINEL).all()


@pytest.mark.parametrize('name', list(oc.CLOUDS))
def test_wrapper_on_hand_clouds(cuda_device, name):
    from catgrasp_amd import my_cpp
    pts, res = oc.CLOUDS[name]()
    ref = co.make_occupancy_grid(pts, res)
    got = my_cpp.makeOccupancyGridFromCloudScan(pts, np.eye(3), res)
    assert len(ref) > 0 and got.dtype == np.float32 and got.shape == ref.shape
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))
