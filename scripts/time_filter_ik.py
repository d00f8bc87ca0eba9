#!/usr/bin/env python
"""filter_ik=True at the bench's C3 size and in the pick cycle: the per-call path (filter_on_device per segment: pre-IK compose, IK kernel,
compose, grid, exhaustive) against FilterPlan.run(ik=...) (fused compose + IK, grid, exhaustive), HIP-event time per filter, alternated in
one process; then pipeline.evaluate_objects(..., ik=...) serial (overlap=None) against the overlapped default (overlap='stages').
usage: python scripts/time_filter_ik.py [out.json] [--trace: two rounds of each filter form only, for a rocprofv3 --kernel-trace pass]"""
import json
import os
import sys
import time
import types

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from catgrasp_amd import pipeline, synth, transforms, workload  # noqa: E402

dev = torch.device('cuda:0')
I4 = np.eye(4)
cam_in_world = np.eye(4); cam_in_world[:3, :3] = [[0, -1, 0], [-1, 0, 0], [0, 0, -1]]; cam_in_world[:3, 3] = [0.55, 0.0, 0.95]
ee_in_grasp = np.eye(4); ee_in_grasp[0, 3] = -0.15
upper = [2.96, 2.09, 2.96, 2.09, 2.96, 2.09, 3.05]; lower = [-u for u in upper]
IK = dict(cam_in_world=cam_in_world, ee_in_grasp=ee_in_grasp, upper=upper, lower=lower)

nets = types.SimpleNamespace(cfg={'n_pts': 2048})
b = workload.SceneBatch(dev, nets, nets, kind='nut', n_objects=8, pts_per_object=2500, per_replica=50000, gripper_subdivisions=4, ik=IK)
rects = [(s, *r) for s, a, c in workload.intersect(b.segs, 0, b.n_total) for r in workload.split_eval_range(s.n_sym, a, c)]
plan_codes, _ = b.run_filter_many('all', rects)
plan = b._plans['all']
g = b.gripper


def per_call():
    return torch.cat([b.run_filter(*r)[0] for r in rects])


def fused():
    return plan.run(g['gripper_in_grasp'], True, keep_rejected_pose=True, ik=IK)[0]


if '--trace' in sys.argv:
    for _ in range(2):
        per_call(); fused()
    torch.cuda.synchronize()
    print('trace rounds 2', plan.E, len(rects))
    sys.exit(0)

c_old, c_new = per_call(), fused()
assert torch.equal(c_old, c_new) and torch.equal(c_new, plan_codes), 'per-call and plan codes differ'
grids = all(sc.grid_open is not None and sc.grid_enc is not None for sc in b.scenes)


def once(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); fn(); e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1)


for _ in range(3):
    once(per_call); once(fused)
t_old, t_new = [], []
for _ in range(25):
    t_old.append(once(per_call)); t_new.append(once(fused))
hist = np.bincount(c_new.cpu().numpy().astype(np.int64), minlength=5).tolist()
out = {'what': 'filter_ik=True over the C3 batch (8 nut objects x {canonical grasps x 12 symmetries, cone poses}; 9,216 / 12,288-triangle '
               'gripper), HIP events around one whole filter, 3 warm-up rounds, 25 alternated rounds, median',
       'evaluations': plan.E, 'segments': len(rects), 'grids': grids, 'code_histogram_0_to_4': hist, 'codes_equal': True,
       'per_call': {'form': 'filter_on_device per segment: compose (ee_out) + iiwa_ik_kernel + compose + grid + exhaustive',
                    'launches': len(rects) * (5 if grids else 4), 'ms_median': round(float(np.median(t_old)), 3),
                    'ms_min': round(float(np.min(t_old)), 3), 'ms_max': round(float(np.max(t_old)), 3)},
       'plan': {'form': 'FilterPlan.run(ik=...): compose_grasp_pose_multi_ik_kernel + grid + exhaustive',
                'launches': 3 if grids else 2, 'ms_median': round(float(np.median(t_new)), 3),
                'ms_min': round(float(np.min(t_new)), 3), 'ms_max': round(float(np.max(t_new)), 3)}}
print(json.dumps(out), flush=True)

# ---- the pick cycle with IK: the bench's pick_cycle_block job (8 C3 objects, 2,000 canonical grasps x 12 symmetries each)
from catgrasp_amd.predicter import DEFAULT_GRASP_CFG, DEFAULT_NUNOCS_CFG, GraspPredicter, NunocsPredicter  # noqa: E402
gp = GraspPredicter('nut', cfg=DEFAULT_GRASP_CFG, state_dict=synth.make_state_dict('cls', 6, 10, seed=0), device=dev)
npred = NunocsPredicter('nut', cfg=DEFAULT_NUNOCS_CFG, state_dict=synth.make_state_dict('seg', 6, 300, seed=1), device=dev)
gg = dict(g)
gg['finger_vertices'] = [gg['vertices'][8:16], gg['vertices'][16:24]]
gg['grip_dirs'] = [[0, -1, 0], [0, 1, 0]]
scene_pts = np.concatenate([o['xyz'] for o in b.objs])
K = np.array([[600, 0, 320], [0, 600, 240], [0, 0, 1.0]])
sym = transforms.get_symmetry_tfs('nut')
rng = np.random.default_rng(11)
canon_pts, canon_nrm = synth.nut_surface(3000, rng)
job = []
for k, ob in enumerate(b.objs):
    grasps = np.linalg.inv(b.nocs_pose[k]) @ synth.make_candidates(ob, 2000, np.random.default_rng(100 + k), gg['hand_depth'], gg['init_bite'])
    job.append({'ob_pts': ob['xyz'], 'ob_normals': ob['normal'], 'symmetry_tfs': sym, 'nocs_pose_override': b.nocs_pose[k],
                'canonical': {'cloud': canon_pts, 'normals': canon_nrm, 'affordance': np.linspace(0, 1, 3000), 'grasps': grasps}})
ik_kw = {'ee_in_grasp': ee_in_grasp, 'upper': upper, 'lower': lower}


def cycle(overlap):
    np.random.seed(0)
    tms = []
    torch.cuda.synchronize(); t0 = time.perf_counter()
    outs = pipeline.evaluate_objects(job, scene_pts, K, gg, gp, npred, draw_ahead=overlap is not None, overlap=overlap, timings=tms, rng='numpy',
                                     cam_in_world=cam_in_world, ik=ik_kw)
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    key = [(o['n_evaluated'], o['poses'].tobytes(), o['p_T_G'].tobytes()) for o in outs]
    st = np.random.get_state()
    return wall / len(job) * 1e3, key, (st[1].tobytes(), st[2]), sum(o['n_evaluated'] for o in outs), sum(len(o['poses']) for o in outs), tms


cycle(None); cycle('stages')                      # warm-up
ms = {None: [], 'stages': []}
ref = {}
for _ in range(3):
    for mode in (None, 'stages'):
        m, key, st, n_eval, n_surv, tms = cycle(mode)
        ms[mode].append(m)
        ref.setdefault(mode, (key, st, n_eval, n_surv, tms))
same = ref[None][0] == ref['stages'][0] and ref[None][1] == ref['stages'][1]
busy = all('stages thread: busy' in t for t in ref['stages'][4])
pick = {'what': "pipeline.evaluate_objects(..., cam_in_world, ik=...) over the 8 C3 objects (2,000 canonical grasps x 12 symmetries + cone "
                "poses each, default settings: rng='numpy', reference RANSAC draws), host clock around the cycle, 1 warm-up + 3 alternated runs, median",
        'evaluations': ref[None][2], 'survivors': ref[None][3], 'results_and_generator_state_equal': same, 'overlapped': busy,
        'serial_ms_per_object': round(float(np.median(ms[None])), 1), 'serial_runs': [round(v, 1) for v in ms[None]],
        'stages_ms_per_object': round(float(np.median(ms['stages'])), 1), 'stages_runs': [round(v, 1) for v in ms['stages']]}
print(json.dumps(pick), flush=True)
res = {'filter_c3_with_ik': out, 'pick_cycle_with_ik': pick, 'device': torch.cuda.get_device_name(0)}
if len(sys.argv) > 1 and not sys.argv[1].startswith('--'):
    os.makedirs(os.path.dirname(sys.argv[1]) or '.', exist_ok=True)
    with open(sys.argv[1], 'w') as f:
        json.dump(res, f, indent=1)
assert same and busy
