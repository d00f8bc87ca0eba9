"""dev: time of one PointGroup training step (catgrasp_amd.pointgroup_train) at the shipped configuration, and of the batch-statistics
BatchNorm + ReLU on its own -> profiles/pointgroup_train_time.json.

  python scripts/pointgroup_train_time.py          on the MI355X: HIP-event times, median of --reps (25) after three warm-up calls

Cloud: the 11,914-voxel bin scene of scripts/sparse_conv_time.py, rows in random order, 16,384 points.  Weights: the constructor's
initialisation (times do not depend on values).

Timed:
  one training step -- forward + offset loss + backward, gradients dropped beforehand -- with the rule books built inside the step and
  over ready rule books;
  the baseline: the SAME network with nn.BatchNorm1d + nn.ReLU + torch indexing + nn.Linear in place of the fused functions
  (pointgroup_train.USE_TORCH_OPS); the sparse layers and their gradients are the same HIP kernels in both.  The two are timed
  alternately, --rounds times each, and every round's median is kept: their spread is what a difference has to exceed;
  BatchNorm + ReLU forward + backward alone on the cloud's 11,914 rows at c = 16 and c = 224, fused and as torch ops, and the fused
  kernels' bytes -- forward 3 reads of x and 1 write of y, backward 2 reads each of x and dy and 1 write of dx, 4 bytes an element --
  over their time, against the 6.3 TB/s that HBM achieves on this part (8 TB/s peak).  At these sizes the rows stay in the caches and
  the time is the five launches': the figure says how far from a bandwidth-bound regime the layer runs, not how good the kernel is.

The clocks `rocm-smi --showclocks` reports after the timed loops are recorded as read."""
import argparse
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.join(HERE, '..')
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
from pointgroup_time import SHIPPED  # noqa: E402
from sparse_conv_time import bin_scene, voxels  # noqa: E402

OUT = os.path.join(ROOT, 'profiles', 'pointgroup_train_time.json')
HBM_ACHIEVABLE = 6.3e12


def main(reps, rounds, out_path):
    import torch
    from torch import nn
    import catgrasp_amd.spconv as spconv
    from catgrasp_amd import batchnorm, pointgroup_train
    dev = torch.device('cuda:0')

    def timed(fn):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); fn(); b.record(); torch.cuda.synchronize()
            ms.append(a.elapsed_time(b))
        return round(statistics.median(ms), 4)

    cfg = argparse.Namespace(**SHIPPED, loss_weight=[1.0, 1.0, 1.0, 1.0], batch_size=1)
    torch.manual_seed(0)
    model = pointgroup_train.PointGroup(cfg).to(dev).train()
    idx_np, shape = voxels(bin_scene())
    idx = torch.from_numpy(idx_np).to(dev)
    n, points = len(idx_np), 16384
    g = torch.Generator().manual_seed(1)
    feats = (torch.rand((n, 6), generator=g) * 2 - 1).to(dev)
    imap = torch.cat((torch.randperm(n, generator=g), torch.randint(n, (points - n,), generator=g)))[torch.randperm(points, generator=g)].int().to(dev)
    v2p = pointgroup_train.v2p_from_input_map(imap, n)
    coords, info = torch.rand((points, 3), generator=g).to(dev), torch.rand((points, 9), generator=g).to(dev)
    books = {}

    def step(ready):
        model.zero_grad(set_to_none=True)
        x = spconv.SparseConvTensor(feats, idx, shape, 1)
        if ready:
            x.indice_dict = books
        ret = model(x, imap, coords, None, None, 0, v2p_map=v2p)
        loss, _, _ = pointgroup_train.loss_fn({'pt_offsets': (ret['pt_offsets'], coords, info, None)}, 0, cfg)
        loss.backward()
        return x, loss

    first, loss = step(False)
    books.update(first.indice_dict)
    data = {'device': torch.cuda.get_device_name(0), 'reps': reps, 'rounds': rounds, 'active_voxels': n, 'points': points, 'spatial_shape': shape,
            'voxels_per_level': [int(books[f'subm{i}'].in_indices.shape[0]) for i in range(1, 8)],
            'timer': 'HIP events around the python calls, median of reps after three warm-up calls; a step is launch-bound, so the times '
                     'include the host side of every launch', 'hbm_achievable_tb_per_s': HBM_ACHIEVABLE / 1e12}
    runs = {'fused': [], 'torch_ops': [], 'fused_ready_rule_books': [], 'torch_ops_ready_rule_books': []}
    losses = {}
    for _ in range(rounds):
        for name, flag in (('fused', False), ('torch_ops', True)):
            pointgroup_train.USE_TORCH_OPS = flag
            runs[name].append(timed(lambda: step(False)))
            runs[name + '_ready_rule_books'].append(timed(lambda: step(True)))
            losses[name] = float(step(True)[1])
    pointgroup_train.USE_TORCH_OPS = False
    for name, ms in runs.items():
        data[f'{name}_step_ms_per_round'] = ms
        data[f'{name}_step_ms'] = round(statistics.median(ms), 4)
    data['spread_between_repeated_medians_ms'] = round(max(max(ms) - min(ms) for ms in runs.values()), 4)
    data['fused_minus_torch_ops_ms'] = round(data['fused_step_ms'] - data['torch_ops_step_ms'], 4)
    data['loss_fused_and_torch_ops'] = [losses['fused'], losses['torch_ops']]

    rows = []
    for c in (16, 224):
        x = (torch.rand((n, c), generator=g) * 2 - 1).to(dev).requires_grad_()
        dy = (torch.rand((n, c), generator=g) * 2 - 1).to(dev)
        bn, relu = nn.BatchNorm1d(c, eps=1e-5, momentum=0.1).to(dev).train(), nn.ReLU()

        def fused():
            x.grad = bn.weight.grad = bn.bias.grad = None
            batchnorm.bn_relu_train(x, bn).backward(dy)

        def torch_ops():
            x.grad = bn.weight.grad = bn.bias.grad = None
            relu(bn(x)).backward(dy)

        xd = x.detach()
        _, stats = batchnorm.bn_relu_forward(xd, bn.weight.detach(), bn.bias.detach(), bn.eps)
        row = {'rows': n, 'c': c}
        for _ in range(rounds):
            row.setdefault('fused_forward_backward_ms_per_round', []).append(timed(fused))
            row.setdefault('torch_ops_forward_backward_ms_per_round', []).append(timed(torch_ops))
        row['fused_forward_backward_ms'] = statistics.median(row['fused_forward_backward_ms_per_round'])
        row['torch_ops_forward_backward_ms'] = statistics.median(row['torch_ops_forward_backward_ms_per_round'])
        row['kernels_forward_ms'] = timed(lambda: batchnorm.bn_relu_forward(xd, bn.weight.detach(), bn.bias.detach(), bn.eps))
        row['kernels_backward_ms'] = timed(lambda: batchnorm.bn_relu_backward(xd, dy, stats))
        for what, passes in (('forward', 4), ('backward', 5)):
            nbytes = passes * n * c * 4
            row[f'{what}_bytes'] = nbytes
            rate = nbytes / (row[f'kernels_{what}_ms'] * 1e-3)
            row[f'{what}_gb_per_s'] = round(rate / 1e9, 2)
            row[f'{what}_fraction_of_achievable_hbm'] = round(rate / HBM_ACHIEVABLE, 5)
        rows.append(row)
        print(row, flush=True)
    data['batchnorm_relu_alone'] = rows
    try:
        lines = subprocess.run(['rocm-smi', '--showclocks'], capture_output=True, text=True, timeout=60).stdout.splitlines()
        data['clocks_after_the_timed_loops'] = [l.strip() for l in lines if 'sclk' in l or 'mclk' in l]
    except Exception as e:          # the tool is not part of the product
        data['clocks_after_the_timed_loops'] = f'not read: {e}'
    print({k: v for k, v in data.items() if k != 'batchnorm_relu_alone'}, flush=True)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, 'w') as f:
        json.dump({'catgrasp_amd_on_mi355x': data}, f, indent=1, sort_keys=True)
        f.write('\n')


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=25)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--out', default=OUT)
    args = ap.parse_args()
    main(args.reps, args.rounds, args.out)
