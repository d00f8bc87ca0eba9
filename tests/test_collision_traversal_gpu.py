"""The grasp filter's traversal on the device, on the single-witness scenes of tests/collision_scenes.py (certified on the CPU by
tests/test_collision_scenes_cpu.py).  Every case and its minus variant runs accelerated (stated key order with block boxes, without boxes,
and through the ordinary Morton-sorted GripperScene), exhaustive, through FilterPlan, and with keep_rejected_pose on and off: each run
must give the constructed codes and nudges and the oracle's pose bits.  work_stats proves reach on the minus variants: the keys read are
those of exactly the blocks the numpy restatement visits, the pairs tested are the queued pairs it counts."""
import copy
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import collision_scenes as cs
from collision_scenes import RES
from oracle import collision_oracle as co

pytestmark = pytest.mark.gpu
I4 = np.eye(4)
CASES = cs.cases()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _oracle(case):
    (V0, F0), (V1, F1) = case.mesh(0), case.mesh(1)
    return co.filter_grasp_pose(case.poses, case.syms, I4, I4, I4, I4, case.gig, 0, 0, case.adjust, V0, F0, V1, F1, case.points(0),
                                case.points(1), RES)


def _set_keys(sc, case, use_blocks=True):
    """the case's voxel sets in the STATED order, with the builder's boxes of every run of 64 (or without boxes)"""
    for side, (ka, ba) in enumerate((('keys_open', 'blocks_open'), ('keys_bg', 'blocks_bg'))):
        k = case.keys[side]
        k4 = np.zeros((len(k), 4), dtype=np.int16); k4[:, :3] = k
        bx = case.boxes(side)
        b4 = np.zeros((len(bx), 2, 4), dtype=np.int16); b4[:, :, :3] = bx
        setattr(sc, ka, torch.from_numpy(k4).to(sc.device))
        setattr(sc, ba, torch.from_numpy(b4).to(sc.device) if use_blocks and len(k) else None)
    return sc


def _scene(case, accel, with_points=False):
    """with_points: the ordinary route -- GripperScene voxelises the case's voxel centres and sorts them through voxel_blocks; otherwise
    the voxel sets are left empty for _set_keys"""
    from catgrasp_amd import my_cpp
    (V0, F0), (V1, F1) = case.mesh(0), case.mesh(1)
    none = np.full((1, 3), 99999.0)
    sc = my_cpp.GripperScene(V0, F0, V1, F1, case.points(0) if with_points else none, case.points(1) if with_points else none, RES,
                             accel=accel, cache=False)
    assert (sc.grid_open is not None) == accel
    if with_points:
        for keys, blocks, k in ((sc.keys_open, sc.blocks_open, case.keys[0]), (sc.keys_bg, sc.blocks_bg, case.keys[1])):
            got = keys[:, :3].cpu().numpy().astype(np.int64)
            assert sorted(map(tuple, got)) == sorted(map(tuple, k)), 'voxelize returns the keys of the case'
            assert blocks.shape[0] == (len(k) + 63) // 64
    return sc


def _direct(sc, case, keep=False, stats=None):
    from catgrasp_amd import my_cpp
    out = my_cpp.filter_on_device(sc, case.poses, case.syms, I4, I4, I4, I4, case.gig, False, False, case.adjust, keep_rejected_pose=keep,
                                  work_stats=stats)
    return tuple(t.cpu().numpy() for t in out)


def _plan(sc, case, keep=False, stats=None):
    from catgrasp_amd import my_cpp
    gp = torch.from_numpy(case.poses.astype(np.float32).reshape(-1, 16)).to(sc.device)
    st = torch.from_numpy(case.syms.astype(np.float32).reshape(-1, 16)).to(sc.device)
    plan = my_cpp.FilterPlan([(sc, gp, st, I4, I4, case.adjust)])
    out = plan.run(case.gig, False, keep_rejected_pose=keep, work_stats=stats)
    return tuple(t.cpu().numpy() for t in out)


def _same(got, exp, what):
    assert np.array_equal(got[0], exp[0]), f'{what}: codes {got[0].tolist()[:8]} expected {exp[0].tolist()[:8]}'
    assert np.array_equal(got[2], exp[2]), f'{what}: nudge {got[2].tolist()[:8]} expected {exp[2].tolist()[:8]}'
    a = np.ascontiguousarray(got[1], dtype=np.float32).view(np.uint32); b = np.ascontiguousarray(exp[1], dtype=np.float32).view(np.uint32)
    assert np.array_equal(a, b), f'{what}: pose bits differ'


@pytest.mark.parametrize('case', CASES, ids=[c.name for c in CASES])
def test_every_route_finds_the_single_witness(cuda_device, case):
    acc, exh = _scene(case, True), (_scene(case, False) if case.routes == 'all' else None)
    for c in [case] + ([case.variant(minus=True)] if case.wit is not None else []):
        what = case.name + (' minus' if c.minus else '')
        exp, kept = c.expected(), c.expected(keep_rejected_pose=True)
        ora = _oracle(c)
        _same(ora, exp, what + ' oracle')
        got = _direct(_set_keys(acc, c), c)
        _same(got, exp, what + ' accelerated')
        if case.routes != 'all':
            continue
        _same(_direct(acc, c, keep=True), kept, what + ' accelerated keep_rejected_pose')
        _same(_plan(acc, c), exp, what + ' FilterPlan')
        _same(_plan(acc, c, keep=True), kept, what + ' FilterPlan keep_rejected_pose')
        _same(_direct(_set_keys(acc, c, use_blocks=False), c), exp, what + ' accelerated, blocks = NULL')
        _same(_plan(acc, c), exp, what + ' FilterPlan, blocks = NULL')
        _same(_direct(_scene(c, True, with_points=True), c), exp, what + ' GripperScene / voxel_blocks route')
        _same(_direct(_set_keys(exh, c), c), exp, what + ' exhaustive')
        _same(_direct(exh, c, keep=True), kept, what + ' exhaustive keep_rejected_pose')
        _same(_plan(exh, c), exp, what + ' exhaustive FilterPlan')


A_CASES = [c for c in CASES if c.group == 'A']


@pytest.mark.parametrize('case', A_CASES, ids=[c.name for c in A_CASES])
def test_mesh_voxels_collide_finds_the_single_witness(cuda_device, case):
    """wave_mesh_voxels_collide through cg_mesh_voxels_collide: the witness triangle at the chunk borders, the witness key first / last"""
    from catgrasp_amd import _lib as L
    V, F = case.mesh(0)
    Vd = torch.from_numpy(V.astype(np.float32)).to(cuda_device); Fd = torch.from_numpy(F).to(cuda_device)
    poses = torch.from_numpy(case.gic().reshape(-1, 16)).to(cuda_device)
    for c, want in ((case, [1, 0]), (case.variant(minus=True), [0, 0])):
        k4 = np.zeros((len(c.keys[0]), 4), dtype=np.int16); k4[:, :3] = c.keys[0]
        keys = torch.from_numpy(k4).to(cuda_device)
        out = torch.full((2,), 7, dtype=torch.uint8, device=cuda_device)
        L.check(L.lib().cg_mesh_voxels_collide(L._p(Vd), L._p(Fd), len(F), L._p(poses), 2, L._p(keys), len(k4), RES, L._p(out), L._stream()),
                'cg_mesh_voxels_collide')
        assert out.cpu().tolist() == want, case.name + (' minus' if c.minus else '')
        assert [int(co.mesh_voxels_collide(V, F, case.gic()[e], c.keys[0], RES)) for e in range(2)] == want


STATS = [c for c in CASES if c.stats]


@pytest.mark.parametrize('case', STATS, ids=[c.name for c in STATS])
def test_work_stats_prove_reach(cuda_device, case):
    """minus variant, one evaluation, one non-empty set, adjust = 0: no early exit shortens the counts"""
    side = case.wit[0]
    c = case.variant(minus=True, adjust=0, first_eval_only=True)
    assert len(c.keys[1 - side]) == 0 and c.E == 1
    nk = len(c.keys[side])
    sc = _scene(case, True)

    def run(fn, use_blocks):
        ws = torch.zeros((3,), dtype=torch.int64, device=cuda_device)
        out = fn(_set_keys(sc, c, use_blocks=use_blocks), c, stats=ws)
        _same(out, c.expected(), case.name)
        return [int(v) for v in ws.cpu().tolist()]
    routes = [('accelerated', _direct, True), ('FilterPlan', _plan, True)] + ([('blocks=NULL', _direct, False)] if case.routes == 'all' else [])
    if case.group == 'F':
        for name, fn, ub in routes:
            ws = run(fn, ub)
            print(f'WORK {case.name} {name}: observed {ws}')
            if case.name == 'F_scale088':
                assert ws[0] > 0 and ws[1] > 0, 'the gate admits s = 0.88: grid work'
            else:
                assert ws == [0, 0, 0], 'the gate refuses the pose: the exhaustive kernel does the work'
        return
    g = None
    for name, fn, ub in routes:
        t = cs.traversal(c, side, use_blocks=ub, g=g)
        g = t['grid']
        ws = run(fn, ub)
        print(f'WORK {case.name} {name}: observed {ws} predicted [{t["work0"]}, {t["work1"]}, {t["work2"]}] blocks visited {len(t["visited"])} of '
              f'{t["nblocks"]}, nk {nk}')
        assert ws[0] == t['work0'], f'{name}: keys read {ws[0]}, the visited blocks hold {t["work0"]}'
        assert ws[2] == t['work2'], f'{name}: pairs tested {ws[2]}, queued pairs {t["work2"]}'
        if not ub:
            assert ws[0] == nk
        elif case.group == 'D' or case.name.startswith('B_block'):
            assert ws[0] < nk, 'culling is the subject'
        if case.name == 'B_beyond_table':
            assert ws[0] == 64 == nk - 262144, 'the blocks beyond the table are read in full, the table blocks are culled'
        if case.group == 'C' and 'onepass' in case.name:
            assert ws[2] > 512
        if case.group == 'C' and case.pairs_total == 1601:
            assert ws[2] > 1536


# ---- group G: the segment table, run by waves that cross segment borders ----------------------------------------------------------------
def _segment_run(device):
    """the plan of cs.segment_table() -> codes, poses, nudge, work_stats (numpy)"""
    from catgrasp_amd import my_cpp
    base, rows = cs.segment_table()
    one = base.variant(first_eval_only=True)
    sw = _set_keys(_scene(one, True), one)
    sm = _set_keys(copy.copy(sw), one.variant(minus=True))
    novox = one.variant(minus=True)
    novox.keys = [k[:0] for k in novox.keys]
    sn = _set_keys(copy.copy(sw), novox)
    scenes = {'wit': sw, 'minus': sm, 'novox': sn}
    total = sum(n for _, n, _ in rows)
    gp_all = torch.from_numpy(np.repeat(one.poses.astype(np.float32).reshape(1, 16), total, axis=0)).to(device)
    st = torch.from_numpy(I4.astype(np.float32).reshape(1, 16)).to(device)
    segs, first = [], 0
    for kind, n, adjust in rows:
        segs.append((scenes[kind], gp_all[first:first + n], st, I4, I4, adjust))
        first += n
    plan = my_cpp.FilterPlan(segs)
    ws = torch.zeros((3,), dtype=torch.int64, device=device)
    codes, poses, nudge = plan.run(one.gig, False, work_stats=ws)
    return codes.cpu().numpy(), poses.cpu().numpy(), nudge.cpu().numpy(), ws.cpu().numpy()


def _child_main(path):
    codes, poses, nudge, ws = _segment_run(torch.device('cuda:0'))
    np.savez(path, codes=codes, poses=poses, nudge=nudge, ws=ws)


def test_segment_table_with_fewer_waves_than_evaluations(cuda_device, tmp_path):
    base, rows = cs.segment_table()
    exp = cs.segment_expected(base, rows)
    assert len(exp[0]) > 3 * 1024, 'at 256 workgroups of 4 waves every wave takes three or more evaluations'
    free = _segment_run(cuda_device)
    _same(free[:3], exp, 'segment table, one wave per evaluation')
    # CATGRASP_AMD_FILTER_BLOCKS_PER_CU is read once per process: a fresh child runs the same plan with 256 workgroups
    out = str(tmp_path / 'child.npz')
    env = dict(os.environ, CATGRASP_AMD_FILTER_BLOCKS_PER_CU='1')
    code = ('import sys; sys.path[:0] = [%r, %r]; import test_collision_traversal_gpu as t; t._child_main(%r)' % (os.path.join(ROOT, 'tests'), ROOT, out))
    flags = ['-s'] if sys.flags.no_user_site else []
    r = subprocess.run([sys.executable] + flags + ['-c', code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    z = np.load(out)
    _same((z['codes'], z['poses'], z['nudge']), exp, 'segment table, 1024 waves')
    assert np.array_equal(z['ws'], free[3]), 'the same work either way'
    print(f'WORK G segment table: {len(rows)} rows, {len(exp[0])} evaluations, work_stats {free[3].tolist()} (1024 waves: {z["ws"].tolist()})')
