"""CPU experiment behind the screened 128 -> 1024 layer: how many (point, channel) pairs a sound bf16x3 screen
leaves to verify, on the bench's networks and inputs.

    python scripts/screen_survivors.py [--kappa-log2 -13.23] [--bound l2|abs] [--candidates 12] [--gain 1.6]

For both categories (nut, screw) and the three 128 -> 1024 layers of the classifier it prints the pairs per candidate and, per
64-point tile behind the first, their mean / p99 / max -- with the per-tile threshold the kernel uses, max(running exact maximum,
the tile's own lower bound).  Bounds: `l2` = kappa * ||w_c|| * ||h_p|| (what the kernel ships), `abs` = kappa * sum_k |w_ck| h_pk."""
import argparse
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
import numpy as np
import torch

from catgrasp_amd import folding, synth
from oracle import pointnet_ref as oref
from oracle import transforms_ref as tref


def bf(x):
    return x.to(torch.bfloat16).to(torch.float32)


def split(x):
    hi = bf(x)
    return hi, bf(x - hi)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--kappa-log2', type=float, default=float(np.log2(folding.SCREEN_KAPPA)))
    ap.add_argument('--bound', choices=('l2', 'abs'), default='l2')
    ap.add_argument('--candidates', type=int, default=12)
    ap.add_argument('--gain', type=float, default=1.6)
    ap.add_argument('--cap', type=int, default=3072, help='list capacity: tiles above it fall back')
    args = ap.parse_args()
    kappa = 2.0 ** args.kappa_log2
    torch.set_num_threads(min(16, torch.get_num_threads()))
    cap, orig = [], oref._conv_bn

    def patched(x, sd, conv, bn, relu):
        if conv.endswith('conv3'):
            w = sd[conv + '.weight'][:, :, 0]
            s = sd[bn + '.weight'] / torch.sqrt(sd[bn + '.running_var'] + 1e-5)
            cap.append((conv, (w * s[:, None]).clone(), x.clone()))
        return orig(x, sd, conv, bn, relu)
    oref._conv_bn = patched
    for kind in ('nut', 'screw'):
        objs = synth.make_scene(8, 2500, seed=0, kind=kind)
        sd = synth.make_state_dict('cls', 6, 10, seed=0, gain=args.gain)
        rng = np.random.default_rng(3)
        xs = []
        for k in range(args.candidates):
            ob = objs[k % 8]
            pose = synth.make_candidates(ob, 1, rng)[0]
            ids = tref.draw_ids(len(ob['xyz']), 2048, rng)
            xs.append(tref.grasp_transform(ob['xyz'].copy(), ob['normal'].copy(), pose, ids)['input'])
        x = torch.from_numpy(np.stack(xs)).float()
        cap.clear()
        oref.pointnet_cls_forward(sd, x)
        for conv, W, h in cap:
            wh, wl = split(W)
            hh, hl = split(h)
            zt = (torch.matmul(wh, hl) + torch.matmul(wl, hh) + torch.matmul(wh, hh)).double()
            if args.bound == 'l2':
                scale = W.double().norm(dim=1)[None, :, None] * h.double().norm(dim=1)[:, None, :]
            else:
                scale = torch.matmul(W.double().abs(), h.double().abs())
            E = kappa * scale + folding.SCREEN_FLOOR
            ub, lb = zt + E, zt - E
            B, C, N = zt.shape
            run = torch.full((B, C), -float('inf'), dtype=torch.float64)
            per_tile = []
            for t in range(N // 64):
                sl = slice(t * 64, (t + 1) * 64)
                thr = torch.maximum(run, lb[:, :, sl].max(2)[0])
                per_tile.append((ub[:, :, sl] >= thr[:, :, None]).sum((1, 2)))
                run = thr            # the exact maximum is at least this; the kernel's rmax can only prune more
            pt = torch.stack(per_tile, 1).double()
            rest = pt[:, 1:].flatten()
            print(f'{kind} {conv} bound {args.bound} kappa 2^{args.kappa_log2:.2f}: pairs/candidate {pt.sum(1).mean():.0f} '
                  f'(share {pt.sum(1).mean() / (C * N):.4f}); tile 0 mean {pt[:, 0].mean():.0f}; tiles >= 1 mean {rest.mean():.0f} '
                  f'p99 {rest.quantile(0.99):.0f} max {rest.max():.0f}; over the cap of {args.cap}: {(rest > args.cap).double().mean():.4f}',
                  flush=True)


if __name__ == '__main__':
    main()
