"""mesh_mesh_collide_kernel and cloud_cloud_collide_kernel (csrc/collision_pairs.hip) on the constructed inputs of tests/pair_scenes.py,
certified on the CPU by tests/test_pair_scenes_cpu.py: the contact catalogues pair by pair and as the single witness inside a 257 x 513
filler scene, the single-witness traversal scenes at every thread, chunk and workgroup position, the capped grid, and the all-pairs
scenes.  Every run goes through the C entry points with a 16-byte buffer whose middle byte is the result: prefilled with 0xFF and with 0,
it must come back exactly 0 or 1 and equal to the constructed verdict, and the 15 bytes around it must be untouched.  Each case has a
minus variant (the witness one lattice step out of contact, or away) whose verdict is False: work that is dropped flips one of the two.

Measured on an MI355X, capped shape 4097 x 61953 (2.5e8 box rejects, nothing found: the whole scan), launch to result: 0.35 ms for the
meshes, 0.22 ms for the clouds (`test_*_capped_grid` prints them as TIME); the whole module takes 8 s."""
import ctypes
import time

import numpy as np
import pytest
import torch

import pair_scenes as ps

pytestmark = pytest.mark.gpu
PATTERN = np.arange(16, dtype=np.uint8) + 0x30
SLOT = 7


def _d(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


class _Mesh:
    """a scene's arrays on the device"""

    def __init__(self, s, dev):
        self.VA, self.FA, self.VB, self.FB = _d(s.VA, dev), _d(s.FA, dev), _d(s.VB, dev), _d(s.FB, dev)
        self.pa, self.pb = _d(s.pose_a.reshape(16), dev), _d(s.pose_b.reshape(16), dev)
        self.na, self.nb = len(s.FA), len(s.FB)


class _Cloud:
    def __init__(self, s, dev):
        self.ka, self.kb, self.rel = _d(s.keys4(0), dev), _d(s.keys4(1), dev), _d(s.rel.reshape(16), dev)
        self.na, self.nb, self.res_a, self.res_b = len(s.keys_a), len(s.keys_b), s.res_a, s.res_b


def _buffer(dev, fill):
    b = PATTERN.copy(); b[SLOT] = fill
    return _d(b, dev)


def _out(buf):
    return ctypes.c_void_p(buf.data_ptr() + SLOT)


def _read(buf, what):
    b = buf.cpu().numpy()
    rest = np.delete(b, SLOT)
    assert np.array_equal(rest, np.delete(PATTERN, SLOT)), f'{what}: bytes around the result changed: {b.tolist()}'
    assert b[SLOT] in (0, 1), f'{what}: result byte {b[SLOT]}'
    return int(b[SLOT])


def _launch_mesh(m, buf, swap=False, na=None, nb=None):
    from catgrasp_amd import _lib as L
    a = (m.VA, m.FA, m.na if na is None else na); b = (m.VB, m.FB, m.nb if nb is None else nb); pa, pb = m.pa, m.pb
    if swap:
        a, b, pa, pb = b, a, pb, pa
    L.check(L.lib().cg_mesh_mesh_collide(L._p(a[0]), L._p(a[1]), a[2], L._p(b[0]), L._p(b[1]), b[2], L._p(pa), L._p(pb), _out(buf), L._stream()),
            'cg_mesh_mesh_collide')


def _launch_cloud(c, buf, na=None, nb=None):
    from catgrasp_amd import _lib as L
    L.check(L.lib().cg_voxels_voxels_collide(L._p(c.ka), c.na if na is None else na, c.res_a, L._p(c.kb), c.nb if nb is None else nb, c.res_b,
                                             L._p(c.rel), _out(buf), L._stream()), 'cg_voxels_voxels_collide')


def _verdicts(dev, scene, fills=(0xFF, 0)):
    """the scene through its entry point once per prefill -> [(fill, result)]"""
    mesh = isinstance(scene, ps.MeshScene)
    d = _Mesh(scene, dev) if mesh else _Cloud(scene, dev)
    out = []
    for fill in fills:
        buf = _buffer(dev, fill)
        (_launch_mesh if mesh else _launch_cloud)(d, buf)
        out.append((fill, _read(buf, scene.name)))
    return out


def _check_all(dev, scenes):
    """every scene and minus variant; all mismatches are reported together"""
    wrong, n = [], 0
    for s0 in scenes:
        for s in s0.with_minus():
            for fill, got in _verdicts(dev, s):
                n += 1
                if got != int(s.verdict):
                    wrong.append(f'{s.name} (prefill {fill:#x}): {got}, constructed {int(s.verdict)}')
    assert not wrong, f'{len(wrong)} of {n} runs differ from the constructed verdict:\n' + '\n'.join(wrong[:40])
    return n


# ---------------------------------------------------------------------------------------------------------------------------------
# the catalogues
@pytest.mark.parametrize('embedded', [False, True], ids=['1x1', 'embedded_257x513'])
def test_triangle_catalogue(cuda_device, embedded):
    n = _check_all(cuda_device, ps.mesh_catalogue_scenes(embedded=embedded))
    print(f'triangle catalogue, {"embedded" if embedded else "1 x 1"}: {n} runs')


@pytest.mark.parametrize('embedded', [False, True], ids=['1x1', 'embedded_257x513'])
def test_cube_catalogue(cuda_device, embedded):
    n = _check_all(cuda_device, ps.cloud_catalogue_scenes(embedded=embedded))
    print(f'cube catalogue, {"embedded" if embedded else "1 x 1"}: {n} runs')


def test_zero_area_face_coplanar_miss(cuda_device):
    """a closed segment that passes a triangle's apex in the triangle's plane: only the segment's own in-plane normal separates them"""
    scenes = [s for s in ps.mesh_catalogue_scenes() if s.cls == 'zero-area-own-normal']
    assert len(scenes) == 4
    _check_all(cuda_device, scenes)


# ---------------------------------------------------------------------------------------------------------------------------------
# traversal
POSITIONS = ps.traversal_positions()
POS_IDS = ['na%d_ia%d_nb%d_ib%d' % p for p in POSITIONS]


@pytest.mark.parametrize('i', range(len(POSITIONS)), ids=POS_IDS)
def test_mesh_traversal_single_witness(cuda_device, i):
    _check_all(cuda_device, [ps.mesh_traversal_scenes()[i]])


@pytest.mark.parametrize('i', range(len(POSITIONS)), ids=POS_IDS)
def test_cloud_traversal_single_witness(cuda_device, i):
    _check_all(cuda_device, [ps.cloud_traversal_scenes()[i]])


CAPPED = ps.capped_positions()
CAP_IDS = ['ia%d_ib%d' % (p[1], p[3]) for p in CAPPED]


def _timed(dev, scene):
    mesh = isinstance(scene, ps.MeshScene)
    d = _Mesh(scene, dev) if mesh else _Cloud(scene, dev)
    out = []
    for fill in (0xFF, 0):
        buf = _buffer(dev, fill)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        (_launch_mesh if mesh else _launch_cloud)(d, buf)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        got = _read(buf, scene.name)
        print(f'TIME {scene.name} prefill {fill:#x}: {dt * 1e3:.3f} ms, result {got}')
        assert got == int(scene.verdict), f'{scene.name} (prefill {fill:#x}): {got}, constructed {int(scene.verdict)}'
        out.append(dt)
    return out


@pytest.mark.parametrize('i', range(len(CAPPED)), ids=CAP_IDS)
def test_mesh_capped_grid(cuda_device, i):
    """4097 x 61953 faces: gx = 17, 243 chunks, per = 2, gy = 122 and the last workgroup of grid.y holds one chunk"""
    s = ps.mesh_capped_scenes()[i]
    for v in s.with_minus():
        _timed(cuda_device, v)


@pytest.mark.parametrize('i', range(len(CAPPED)), ids=CAP_IDS)
def test_cloud_capped_grid(cuda_device, i):
    s = ps.cloud_capped_scenes()[i]
    for v in s.with_minus():
        _timed(cuda_device, v)


def test_all_pairs_hit(cuda_device):
    """every workgroup finds a pair at once: the early-exit poll runs with the flag already set by other workgroups"""
    for s in (ps.mesh_self_scene(), ps.cloud_self_scene()):
        for _ in range(3):
            assert _verdicts(cuda_device, s) == [(0xFF, 1), (0, 1)], s.name


def test_empty_side_clears_a_prefilled_byte(cuda_device):
    m = _Mesh(ps.mesh_traversal_scenes()[5], cuda_device)
    c = _Cloud(ps.cloud_traversal_scenes()[5], cuda_device)
    for na, nb in ((0, None), (None, 0), (0, 0)):
        for fill in (0xFF, 1, 0):
            buf = _buffer(cuda_device, fill)
            _launch_mesh(m, buf, na=na, nb=nb)
            assert _read(buf, 'empty mesh') == 0
            buf = _buffer(cuda_device, fill)
            _launch_cloud(c, buf, na=na, nb=nb)
            assert _read(buf, 'empty cloud') == 0


# ---------------------------------------------------------------------------------------------------------------------------------
# symmetry
def test_mesh_verdict_is_symmetric_on_one_stream(cuda_device):
    """A against B and B against A, queued back to back on the same stream, each with its own result buffer"""
    scenes = [ps.mesh_traversal_scenes()[i] for i in (3, 11, 19)] + [s for s in ps.mesh_catalogue_scenes(embedded=True)[::23]]
    for s0 in scenes:
        for s in s0.with_minus():
            m = _Mesh(s, cuda_device)
            b1, b2 = _buffer(cuda_device, 0xFF), _buffer(cuda_device, 0xFF)
            _launch_mesh(m, b1); _launch_mesh(m, b2, swap=True)
            assert _read(b1, s.name) == _read(b2, s.name + ' swapped') == int(s.verdict), s.name


def test_cloud_verdict_is_symmetric_on_one_stream(cuda_device):
    """B against A under inv(rel) (signed-permutation rel: the inverse is exact)"""
    scenes = [s for s in ps.cloud_traversal_scenes() if s.pair.exact][::3] + [s for s in ps.cloud_catalogue_scenes(embedded=True) if s.pair.exact][::7]
    assert len(scenes) >= 8
    for s0 in scenes:
        for s in s0.with_minus():
            c = _Cloud(s, cuda_device)
            inv = ps.exact32(np.linalg.inv(s.rel.astype(np.float64)))
            r = _Cloud(ps.CloudScene(s.name + ' swapped', s.cls, s.keys_b, s.keys_a, s.res_a, inv, s.verdict, res_a=s.res_b), cuda_device)
            b1, b2 = _buffer(cuda_device, 0xFF), _buffer(cuda_device, 0xFF)
            _launch_cloud(c, b1); _launch_cloud(r, b2)
            assert _read(b1, s.name) == _read(b2, s.name + ' swapped') == int(s.verdict), s.name


# ---------------------------------------------------------------------------------------------------------------------------------
# through CollisionManager
def _far_mesh():
    V = np.array([[0, 0, 0], [8, 0, 0], [0, 8, 0]], dtype=np.float32) * np.float32(ps.RES)
    T = np.eye(4, dtype=np.float32); T[:3, 3] = [0.5, 0.5, 0.5]
    return V, np.array([[0, 1, 2]], dtype=np.int32), T


def test_collision_manager_mesh_pairs(cuda_device):
    from catgrasp_amd import my_cpp
    one = {s.pair.name: s for s in ps.mesh_catalogue_scenes()}
    scenes = [one[n] for n in ('pierce', 'vertex_on_face', 'vertex_on_edge_ba', 'edges_cross', 'coplanar_vertex', 'segment_past_apex',
                               'segment_past_apex_ba', 'sole7_r12', 'sole14_ba_r20')] + [ps.mesh_traversal_scenes()[i] for i in (10, 18)]
    n = 0
    for s0 in scenes:
        for s in s0.with_minus():
            cm = my_cpp.CollisionManager()
            a = cm.registerMesh(s.VA, s.FA); b = cm.registerMesh(s.VB, s.FB)
            cm.setTransform(s.pose_a, a); cm.setTransform(s.pose_b, b)
            assert cm.isAnyCollision() == s.verdict, s.name
            n += 1
    assert n >= 20
    # three objects: only the LAST pair (1, 2) collides
    s0 = ps.mesh_traversal_scenes()[13]
    Vf, Ff, Tf = _far_mesh()
    for s in s0.with_minus():
        cm = my_cpp.CollisionManager()
        f = cm.registerMesh(Vf, Ff); a = cm.registerMesh(s.VA, s.FA); b = cm.registerMesh(s.VB, s.FB)
        cm.setTransform(Tf, f); cm.setTransform(s.pose_a, a); cm.setTransform(s.pose_b, b)
        assert cm.isAnyCollision() == s.verdict, s.name + ' (three objects)'


def _register_cloud(cm, keys, res, pose):
    i = cm.registerPointCloud(ps.exact32(ps.centres(keys, res)), res)
    got = cm._obs[i]['keys'][:, :3].cpu().numpy().astype(np.int64)
    assert sorted(map(tuple, got)) == sorted(map(tuple, keys)), 'voxelize returns the keys of the case'
    cm.setTransform(pose, i)
    return i


def test_collision_manager_cloud_pairs(cuda_device):
    """proper rotations only (setTransform refuses a reflected cloud): pose_b = pose_a . rel, so that inv(pose_a) . pose_b is rel bit for bit"""
    from catgrasp_amd import my_cpp
    one = {s.pair.name: s for s in ps.cloud_catalogue_scenes()}
    names = ['face_eq_rel0', 'edge_eq_rel1', 'corner_2to1_rel0', 'corner_x_2to1_rel1', 'inside_2to1_rel1', 'identical_eq_rel0', 'face_2to1_rel0_int16',
             'corner_eq_rel1_int16', 'rot_axis3', 'rot_axis10']
    scenes = [one[n] for n in names] + [s for s in ps.cloud_traversal_scenes()[8:11] if s.pair.proper]
    n = 0
    for s0 in scenes:
        assert s0.pair.proper
        for s in s0.with_minus():
            pose_a = ps.POSE_A if s.pair.exact else np.eye(4)
            pose_b = (pose_a @ s.rel.astype(np.float64)).astype(np.float32)
            rel = (np.linalg.inv(pose_a.astype(np.float32).astype(np.float64)) @ pose_b.astype(np.float64)).astype(np.float32)
            assert np.array_equal(rel, s.rel), s.name
            cm = my_cpp.CollisionManager()
            _register_cloud(cm, s.keys_a, s.res_a, pose_a); _register_cloud(cm, s.keys_b, s.res_b, pose_b)
            assert cm.isAnyCollision() == s.verdict, s.name
            n += 1
    assert n >= 20
    s0 = [s for s in ps.cloud_traversal_scenes() if s.pair.exact and s.pair.proper][4]
    for s in s0.with_minus():
        cm = my_cpp.CollisionManager()
        _register_cloud(cm, np.array([[20000, 20000, 20000]]), s.res_a, np.eye(4))
        _register_cloud(cm, s.keys_a, s.res_a, ps.POSE_A); _register_cloud(cm, s.keys_b, s.res_b, (ps.POSE_A @ s.rel.astype(np.float64)).astype(np.float32))
        assert cm.isAnyCollision() == s.verdict, s.name + ' (three objects)'
