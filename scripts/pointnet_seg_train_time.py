"""dev: time and memory of one NUNOCS training step of PointNetSeg (catgrasp_amd.pointnet2_train) at the training shape of
trainer_nunocs.py -- B = 34 clouds of N = 8192 points, 300 logits per point -- and of its per-point head alone
-> profiles/pointnet_seg_train_time.json.

  python scripts/pointnet_seg_train_time.py          on the MI355X: HIP-event times, median of --reps (10) after two warm-up calls

Weights: the constructor's initialisation (times do not depend on values).  Input: normal points.  Every timed call allocates its
activations, workspaces and gradients afresh through torch's caching allocator (warm after the warm-up calls).

Timed, forward + backward, gradients dropped beforehand, the three variants alternately --rounds times (every round's median is kept:
their spread is what a difference has to exceed):
  head    the per-point head alone on a ready global feature g (B, 1024) and per-point feature (B, N, 64), gradients to both:
            hip        dense_autograd.seg_head_train
            torch_ops  pointnet2_train.PointNetSeg._torch_head: the (B, 1088, N) concatenation, Conv1d, BatchNorm1d, relu -- the
                       arithmetic of the parent's pointnet2.PointNetSeg training forward, whose head this is line for line
  step    the whole model with loss.NocsMinSymmetryCELoss on the device:
            hip, torch_ops (pointnet2_train.USE_TORCH_OPS) and parent (pointnet2.PointNetSeg in training mode)
  peak    torch.cuda.max_memory_allocated() over one call minus the bytes allocated before it (inputs and parameters)
  pieces  every launch group of the HIP head on its own at the head's shapes: forward GEMM (with the device-side packing), BatchNorm +
          ReLU forward and backward, input gradient, weight + bias gradient, group sums.  For the weight gradient at (Cin, Cout) =
          (512, 256) and (64, 512): flops 2 n Cin Cout over its time against the 157.3 TFLOPS of the f32 MFMA, and the bytes it must
          move (x and dy once, the partials written and read once) over its time against the 6.3 TB/s that HBM achieves.

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

OUT = os.path.join(ROOT, 'profiles', 'pointnet_seg_train_time.json')
MFMA_F32_PEAK = 157.3e12
HBM_ACHIEVABLE = 6.3e12


def main(reps, rounds, out_path, B, N, n_out):
    import torch
    from torch import nn
    from catgrasp_amd import batchnorm, dense_autograd as D, loss as nl, pointnet2, pointnet2_train
    dev = torch.device('cuda:0')

    def timed(fn, warm=2):
        for _ in range(warm):
            fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); fn(); b.record(); torch.cuda.synchronize()
            ms.append(a.elapsed_time(b))
        return round(statistics.median(ms), 4)

    def peak(fn):
        fn()
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        fn()
        torch.cuda.synchronize()
        return int(torch.cuda.max_memory_allocated() - before)

    torch.manual_seed(0)
    ours = pointnet2_train.PointNetSeg(6, n_out).to(dev).train()
    parent = pointnet2.PointNetSeg(6, n_out).to(dev).train()
    parent.load_state_dict(ours.state_dict())
    crit = nl.NocsMinSymmetryCELoss({'nocs_class_name': 'nut', 'ce_loss_bins': n_out // 3})
    g = torch.Generator().manual_seed(1)
    x = (torch.randn((B, N, 6), generator=g) * 0.5).to(dev)
    target = torch.rand((B, N, 3), generator=g).to(dev)
    gf = torch.randn((B, 1024), generator=g).to(dev).requires_grad_()
    pf = torch.randn((B, N, 64), generator=g).to(dev).requires_grad_()
    dl = (torch.randn((B, N, n_out), generator=g) / (B * N) ** 0.5).to(dev)
    convs, bns = (ours.conv1, ours.conv2, ours.conv3, ours.conv4), (ours.bn1, ours.bn2, ours.bn3)

    def head(hip):
        ours.zero_grad(set_to_none=True)
        gf.grad = pf.grad = None
        out = D.seg_head_train(gf, pf, convs, bns) if hip else ours._torch_head(gf, pf)
        out.backward(dl)

    def step(model, torch_ops=False):
        pointnet2_train.USE_TORCH_OPS = torch_ops
        model.zero_grad(set_to_none=True)
        logits, _ = model(x)
        loss = crit(logits, target)
        loss.backward()
        pointnet2_train.USE_TORCH_OPS = False
        return loss

    variants = {'head_hip': lambda: head(True), 'head_torch_ops': lambda: head(False), 'step_hip': lambda: step(ours),
                'step_torch_ops': lambda: step(ours, True), 'step_parent': lambda: step(parent)}
    data = {'device': torch.cuda.get_device_name(0), 'reps': reps, 'rounds': rounds, 'B': B, 'N': N, 'n_out': n_out, 'rows': B * N,
            'timer': 'HIP events around the python calls, median of reps after two warm-up calls; every call allocates its activations, '
                     'workspaces and gradients afresh from the warm caching allocator',
            'mfma_f32_peak_tflops': MFMA_F32_PEAK / 1e12, 'hbm_achievable_tb_per_s': HBM_ACHIEVABLE / 1e12}
    runs = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            runs[k].append(timed(fn))
            print(k, runs[k][-1], flush=True)
    for k, ms in runs.items():
        data[f'{k}_ms_per_round'] = ms
        data[f'{k}_ms'] = round(statistics.median(ms), 4)
    data['spread_between_repeated_medians_ms'] = round(max(max(ms) - min(ms) for ms in runs.values()), 4)
    for k, fn in variants.items():
        data[f'{k}_peak_bytes_above_inputs'] = peak(fn)
    data['loss_hip_torch_ops_parent'] = [float(step(ours)), float(step(ours, True)), float(step(parent))]

    n = B * N
    pieces = []
    for cin, cout, rows, rpg in ((64, 512, n, N), (1024, 512, B, 0), (512, 256, n, 0), (256, 128, n, 0), (128, n_out, n, 0)):
        xx = torch.randn((rows, cin), generator=g).to(dev)
        dy = (torch.randn((rows, cout), generator=g) / rows ** 0.5).to(dev)
        w = (torch.randn((cout, cin), generator=g) / cin ** 0.5).to(dev)
        b = torch.zeros(cout, device=dev)
        rb = torch.zeros((rows // rpg, cout), device=dev) if rpg else None
        row = {'cin': cin, 'cout': cout, 'rows': rows,
               'forward_ms': timed(lambda: D.dense_forward(xx, w, None if rpg else b, rb, rpg or 1)),
               'pack_b_ms': timed(lambda: D.pack_b(w)),
               'dgrad_ms': timed(lambda: D.dense_dgrad(dy, w)),
               'wgrad_ms': timed(lambda: D.dense_wgrad(xx, dy))}
        if rpg:
            row['group_sums_ms'] = timed(lambda: D.group_sums(dy, rpg))
        flops = 2.0 * rows * cin * cout
        chunks = -(-rows // D.grad_rows())
        nbytes = 4.0 * (rows * (cin + cout) + 2 * chunks * (cin * cout + cout) + cin * cout + cout)
        for what in ('forward', 'dgrad', 'wgrad'):
            row[f'{what}_tflops'] = round(flops / (row[f'{what}_ms'] * 1e-3) / 1e12, 2)
            row[f'{what}_fraction_of_mfma_f32_peak'] = round(flops / (row[f'{what}_ms'] * 1e-3) / MFMA_F32_PEAK, 4)
        row['wgrad_bytes'] = nbytes
        row['wgrad_fraction_of_achievable_hbm'] = round(nbytes / (row['wgrad_ms'] * 1e-3) / HBM_ACHIEVABLE, 4)
        if rows == n and cout % 16 == 0:
            bn = nn.BatchNorm1d(cout).to(dev).train()
            z = torch.randn((rows, cout), generator=g).to(dev)
            _, stats = batchnorm.bn_relu_forward(z, bn.weight.detach(), bn.bias.detach(), bn.eps)
            row['bn_relu_forward_ms'] = timed(lambda: batchnorm.bn_relu_forward(z, bn.weight.detach(), bn.bias.detach(), bn.eps))
            row['bn_relu_backward_ms'] = timed(lambda: batchnorm.bn_relu_backward(z, dy, stats))
        pieces.append(row)
        print(row, flush=True)
        del xx, dy, w
    data['pieces_of_the_hip_head'] = pieces
    try:
        lines = subprocess.run(['rocm-smi', '--showclocks'], capture_output=True, text=True, timeout=60).stdout.splitlines()
        data['clocks_after_the_timed_loops'] = [l.strip() for l in lines if 'sclk' in l or 'mclk' in l]
    except Exception as e:          # the tool is not part of the product
        data['clocks_after_the_timed_loops'] = f'not read: {e}'
    print({k: v for k, v in data.items() if k != 'pieces_of_the_hip_head'}, flush=True)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, 'w') as f:
        json.dump({'catgrasp_amd_on_mi355x': data}, f, indent=1, sort_keys=True)
        f.write('\n')


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--batch', type=int, default=34)
    ap.add_argument('--points', type=int, default=8192)
    ap.add_argument('--n-out', type=int, default=300)
    ap.add_argument('--out', default=OUT)
    args = ap.parse_args()
    main(args.reps, args.rounds, args.out, args.batch, args.points, args.n_out)
