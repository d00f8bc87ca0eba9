"""dev: time and memory of PointNet's pooled layer Conv1d(128 -> 1024, k = 1) + BatchNorm1d (batch statistics) + [ReLU] + max over the
points in training mode, closed form on HIP (catgrasp_amd.pool_autograd.conv_bn_max_train) against the torch composite, and of one
NUNOCS training step of PointNetSeg with pointnet2_train.ENCODER_ON_HIP off and on, at the training shape of trainer_nunocs.py --
B = 34 clouds of N = 8192 points -> profiles/pool_train_time.json.

  python scripts/pool_train_time.py          on the MI355X: HIP-event times, median of --reps (10) after two warm-up calls

Timed, forward + backward, gradients dropped beforehand, the variants alternately --rounds times (every round's median is kept: their
spread is what a difference has to exceed):
  layer   one pooled layer on a ready (B, N, 128) input with gradients to the input and every parameter, with and without ReLU:
            hip        pool_autograd.conv_bn_max_train
            torch_ops  Conv1d -> BatchNorm1d -> [relu] -> max(dim = 2) on a contiguous (B, 128, N) leaf: the parent's arithmetic for this layer
  step    the whole model with loss.NocsMinSymmetryCELoss on the device, the switch off (the default: the encoder on torch ops) and on
  peak    torch.cuda.max_memory_allocated() over one call minus the bytes allocated before it (inputs and parameters, gradients dropped)
  pieces  the launch groups of the closed form on their own: centred Gram matrix, extrema, mean, variance sweep, statistics, gather,
          scatter.
  kappa   for the three pooled layers of the model at this shape (constructor weights, normal points): the inputs are caught with
          forward hooks on a torch-op forward, and per channel kappa = |W[c]|^2 lambda_max(S) / (M var[c]) is computed in float64 --
          the factor by which the variance from the Gram matrix loses accuracy (tests/pool_train_ref.py: kappa); max and median.

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

OUT = os.path.join(ROOT, 'profiles', 'pool_train_time.json')
MFMA_F32_PEAK = 157.3e12


def main(reps, rounds, out_path, B, N, n_out, cin, c):
    import torch
    import torch.nn.functional as F
    from torch import nn
    from catgrasp_amd import loss as nl, pointnet2_train, pool_autograd as PA
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
        clear()                                 # the gradients of the warm-up call are no inputs
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        fn()
        torch.cuda.synchronize()
        return int(torch.cuda.max_memory_allocated() - before)

    torch.manual_seed(0)
    g = torch.Generator().manual_seed(1)
    conv, bn = nn.Conv1d(cin, c, 1).to(dev).train(), nn.BatchNorm1d(c).to(dev).train()
    with torch.no_grad():
        bn.weight.add_(0.2 * torch.randn(c, generator=g).to(dev)); bn.weight[::7].neg_()
    h = torch.randn((B, N, cin), generator=g).to(dev).requires_grad_()
    ht = h.detach().transpose(1, 2).contiguous().requires_grad_()      # the baseline's own leaf, channel-major as the parent's tensor is
    dout = torch.randn((B, c), generator=g).to(dev)

    def layer(hip, relu):
        clear()
        if hip:
            out = PA.conv_bn_max_train(h, conv, bn, relu)
        else:
            y = bn(conv(ht))
            out = (F.relu(y) if relu else y).max(dim=2)[0]
        out.backward(dout)

    model = pointnet2_train.PointNetSeg(6, n_out).to(dev).train()
    crit = nl.NocsMinSymmetryCELoss({'nocs_class_name': 'nut', 'ce_loss_bins': n_out // 3})
    x = (torch.randn((B, N, 6), generator=g) * 0.5).to(dev)
    target = torch.rand((B, N, 3), generator=g).to(dev)

    def clear():
        conv.zero_grad(set_to_none=True); bn.zero_grad(set_to_none=True); model.zero_grad(set_to_none=True)
        h.grad = ht.grad = None

    def step(on):
        pointnet2_train.ENCODER_ON_HIP = on
        try:
            clear()
            logits, _ = model(x)
            loss = crit(logits, target)
            loss.backward()
        finally:
            pointnet2_train.ENCODER_ON_HIP = False
        return loss

    variants = {'layer_relu_hip': lambda: layer(True, True), 'layer_relu_torch_ops': lambda: layer(False, True),
                'layer_hip': lambda: layer(True, False), 'layer_torch_ops': lambda: layer(False, False),
                'step_encoder_on_torch_ops': lambda: step(False), 'step_encoder_on_hip': lambda: step(True)}
    data = {'device': torch.cuda.get_device_name(0), 'reps': reps, 'rounds': rounds, 'B': B, 'N': N, 'n_out': n_out, 'cin': cin, 'c': c, 'rows': B * N,
            'timer': 'HIP events around the python calls, median of reps after two warm-up calls of every variant; every call allocates its '
                     'activations, workspaces and gradients afresh from the warm caching allocator',
            'mfma_f32_peak_tflops': MFMA_F32_PEAK / 1e12}
    runs = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            runs[k].append(timed(fn))
            print(k, runs[k][-1], flush=True)
    for k, ms in runs.items():
        data[f'{k}_ms_per_round'] = ms
        data[f'{k}_ms'] = round(statistics.median(ms), 4)
    data['spread_between_repeated_medians_ms'] = {k: round(max(ms) - min(ms), 4) for k, ms in runs.items()}
    for k, fn in variants.items():
        data[f'{k}_peak_bytes_above_inputs'] = peak(fn)
    data['loss_switch_off_on'] = [float(step(False).detach()), float(step(True).detach())]

    hd, w, b = h.detach(), conv.weight.detach().squeeze(2).contiguous(), conv.bias.detach()
    gamma, beta = bn.weight.detach(), bn.bias.detach()
    xbar, s = PA.centred_gram(hd.view(B * N, cin))
    zsel, idx = PA.pool_extrema(hd, w, b, gamma)
    coef = torch.randn((B, c), generator=g).to(dev)
    dx = torch.zeros_like(hd)
    mean = PA.pool_mean(w, b, xbar, B, N)
    var = PA.pool_var(hd, w, b, mean)
    pieces = {'centred_gram_ms': timed(lambda: PA.centred_gram(hd.view(B * N, cin))),
              'mean_ms': timed(lambda: PA.pool_mean(w, b, xbar, B, N)),
              'var_sweep_ms': timed(lambda: PA.pool_var(hd, w, b, mean)),
              'stats_from_gram_ms': timed(lambda: PA.pool_stats(w, b, xbar, s, gamma, beta, bn.eps, N, zsel, True)),
              'extrema_ms': timed(lambda: PA.pool_extrema(hd, w, b, gamma)),
              'stats_ms': timed(lambda: PA.pool_stats(w, b, xbar, None, gamma, beta, bn.eps, N, zsel, True, var=var)),
              'wgrad_gather_ms': timed(lambda: PA.pool_wgrad_gather(hd, coef, idx)),
              'dgrad_scatter_ms': timed(lambda: PA.pool_dgrad_scatter(dx, coef, idx, w))}
    flops = 2.0 * B * N * cin * c
    pieces['extrema_tflops'] = round(flops / (pieces['extrema_ms'] * 1e-3) / 1e12, 2)
    pieces['extrema_fraction_of_mfma_f32_peak'] = round(flops / (pieces['extrema_ms'] * 1e-3) / MFMA_F32_PEAK, 4)
    data['pieces_of_the_closed_form'] = pieces
    gram_var = PA.pool_stats(w, b, xbar, s, gamma, beta, bn.eps, N, zsel, True)[0][1]
    data['relative_difference_of_var_gram_route_vs_sweep_timed_layer'] = float(((gram_var - var).abs() / var).max())

    caught = {}
    layers = {'feat.stn.conv3': model.feat.stn.conv3, 'feat.fstn.conv3': model.feat.fstn.conv3, 'feat.conv3': model.feat.conv3}
    hooks = [m.register_forward_hook(lambda mod, inp, out, k=k: caught.__setitem__(k, inp[0].detach())) for k, m in layers.items()]
    pointnet2_train.USE_TORCH_OPS = True
    try:
        with torch.no_grad():
            model(x)
    finally:
        pointnet2_train.USE_TORCH_OPS = False
        for hk in hooks:
            hk.remove()
    kap = {}
    for k, m in layers.items():
        a = caught[k].double().transpose(1, 2).reshape(B * N, -1)           # (B, Cin, N) -> rows
        a = a - a.mean(0)
        sm = a.t() @ a
        wd = m.weight.detach().double().squeeze(2)
        v = ((wd @ sm) * wd).sum(1) / (B * N)
        kk = (wd * wd).sum(1) * torch.linalg.eigvalsh(sm).max() / (B * N * v)
        lam = torch.linalg.eigvalsh(sm)
        kap[k] = {'kappa_max': float(kk.max()), 'kappa_median': float(kk.median()), 'gram_eigenvalue_max_over_min': float(lam.max() / lam.min().clamp_min(1e-300)),
                  'var_min': float(v.min())}
    data['kappa_of_the_pooled_layers'] = kap
    del caught
    try:
        lines = subprocess.run(['rocm-smi', '--showclocks'], capture_output=True, text=True, timeout=60).stdout.splitlines()
        data['clocks_after_the_timed_loops'] = [l.strip() for l in lines if 'sclk' in l or 'mclk' in l]
    except Exception as e:          # the tool is not part of the product
        data['clocks_after_the_timed_loops'] = f'not read: {e}'
    print(data, flush=True)
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
    ap.add_argument('--cin', type=int, default=128)
    ap.add_argument('--c', type=int, default=1024)
    ap.add_argument('--out', default=OUT)
    args = ap.parse_args()
    main(args.reps, args.rounds, args.out, args.batch, args.points, args.n_out, args.cin, args.c)
