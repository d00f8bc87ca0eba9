"""dev: time of the sparse convolution layers (catgrasp_amd.spconv) on a synthetic bin scene -> profiles/sparse_conv_time.json.

  python scripts/sparse_conv_time.py          on the MI355X: HIP-event times, median of --reps after a warm-up

Cloud: 16,384 points of a bin scene (a floor and a dozen bumps: a surface, as a depth camera sees it), voxelised at 500 voxels
per metre like the reference (config_pointgroup.yaml `scale: 500`), about 12k active voxels.  Everything is measured for two row
orders of the same voxels: a random permutation, and ascending linear key (rows that are neighbours in the grid are then
neighbours in the table, which is what lets the kernel skip offsets that a whole 32-row tile lacks).

Timed: the three rule-book builds, and per channel width (m = 16: 16->16, 32->16, 96->96, 192->96) SubM k = 3, the strided and
the inverse layer, each as ONE launch of the fused kernel.  Beside each, the same layer over the SAME rule book written as the
reference's op sequence in torch on the same device: per offset, index_select -> mm -> index_add_ on the pairs that exist (the
pair lists are made before the clock starts, as the reference's rule book holds them).  That column is independent code, not the
kernel under test; the script also reports the largest difference between the two."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, 'profiles', 'sparse_conv_time.json')
WIDTHS = ((16, 16), (32, 16), (96, 96), (192, 96))
SCALE = 500


def bin_scene(n=16384, seed=16):
    """Points on the visible surface of a 30 x 20 cm bin floor with 12 bumps up to 4 cm high; metres."""
    rng = np.random.default_rng(seed)
    xy = rng.uniform(0, 1, (n, 2)) * (0.30, 0.20)
    z = np.zeros(n)
    for cx, cy, r, hgt in zip(rng.uniform(0.03, 0.27, 12), rng.uniform(0.03, 0.17, 12), rng.uniform(0.012, 0.03, 12), rng.uniform(0.01, 0.04, 12)):
        d2 = (xy[:, 0] - cx) ** 2 + (xy[:, 1] - cy) ** 2
        z = np.maximum(z, hgt * np.sqrt(np.clip(1 - d2 / r ** 2, 0, None)))
    return np.column_stack([xy, z + rng.normal(0, 0.0005, n)])


def voxels(pts):
    v = np.floor((pts - pts.min(0)) * SCALE).astype(np.int64)
    v = np.unique(v, axis=0)
    shape = np.clip(v.max(0) + 1, 128, None)                     # the reference clips the grid to at least full_scale[0] = 128
    idx = np.concatenate([np.zeros((len(v), 1), np.int64), v], axis=1).astype(np.int32)
    return idx[np.random.default_rng(1).permutation(len(idx))], [int(s) for s in shape]


def main(reps, out_path):
    import torch
    import catgrasp_amd.spconv as spconv
    dev = torch.device('cuda:0')

    def timed(fn):
        fn(); torch.cuda.synchronize()
        ms = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); out = fn(); b.record(); torch.cuda.synchronize()
            ms.append(a.elapsed_time(b))
        return round(statistics.median(ms), 4), out

    def pairs(nbr):
        """[(k, output rows, input rows)] of the offsets that have pairs: the reference's indice_pairs, from the same table"""
        res = []
        for k in range(nbr.shape[1]):
            o = torch.nonzero(nbr[:, k] >= 0).flatten()
            if o.numel():
                res.append((k, o, nbr[o, k].long()))
        return res

    def torch_layer(x, plist, w, bias, n_out):
        out = torch.zeros((n_out, w.shape[2]), dtype=torch.float32, device=dev)
        for k, o, i in plist:
            out.index_add_(0, o, torch.mm(x.index_select(0, i), w[k]))
        return out + bias

    def measure(idx_np, shape):
        idx = torch.from_numpy(idx_np).to(dev)
        n = len(idx_np)
        res = {}
        res['rules_subm_ms'], subm = timed(lambda: spconv.subm_rules(idx, shape, 1))
        res['rules_down_ms'], down = timed(lambda: spconv.down_rules(idx, shape, 1))

        def inverse():
            down.extra.pop('inverse_nbr', None)
            return spconv.inverse_rules(down)
        res['rules_inverse_ms'], inv = timed(inverse)
        m = down.out_indices.shape[0]
        res['strided_outputs'] = m
        res['neighbours_per_site_of_27'] = round(float((subm.nbr >= 0).float().mean()) * 27, 2)
        tiles = subm.nbr.view(-1)[:(n // 32) * 32 * 27].view(n // 32, 32, 27)
        res['offsets_present_per_32_row_tile_of_27'] = round(float((tiles >= 0).any(1).float().sum(1).mean()), 2)
        layers = []
        g = torch.Generator(device='cpu').manual_seed(0)
        for cin, cout in WIDTHS:
            row = {'cin': cin, 'cout': cout}
            for kind, nbr, n_in, n_out, K in (('subm3', subm.nbr, n, n, 27), ('strided', down.nbr, n, m, 8), ('inverse', inv, m, n, 8)):
                x = (torch.rand((n_in, cin), generator=g) * 2 - 1).to(dev)
                w = ((torch.rand((K, cin, cout), generator=g) * 2 - 1) * (3.0 / cin) ** 0.5).to(dev)
                bias = (torch.rand((cout,), generator=g) * 2 - 1).to(dev)
                plist = pairs(nbr)
                row[f'{kind}_fused_ms'], got = timed(lambda: spconv.sparse_conv(x, nbr, w, bias))
                row[f'{kind}_torch_ops_ms'], want = timed(lambda: torch_layer(x, plist, w, bias, n_out))
                row[f'{kind}_torch_launches'] = 3 * len(plist) + 2
                row[f'{kind}_max_abs_difference'] = float((got - want).abs().max())
            layers.append(row)
            print(row, flush=True)
        res['layers'] = layers
        print({k: v for k, v in res.items() if k != 'layers'}, flush=True)
        return res

    idx_np, shape = voxels(bin_scene())
    key = ((idx_np[:, 1].astype(np.int64) * shape[1]) + idx_np[:, 2]) * shape[2] + idx_np[:, 3]
    data = {'device': torch.cuda.get_device_name(0), 'reps': reps, 'timer': 'HIP events, median; the rule-book times include their host reads of the error flag',
            'points': 16384, 'voxels_per_metre': SCALE, 'active_voxels': len(idx_np), 'spatial_shape': shape}
    with torch.no_grad():
        data['rows_in_random_order'] = measure(idx_np, shape)
        data['rows_in_key_order'] = measure(idx_np[np.argsort(key)], shape)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, 'w') as f:
        json.dump({'catgrasp_amd_on_mi355x': data}, f, indent=1, sort_keys=True)
        f.write('\n')


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out', default=OUT)
    args = ap.parse_args()
    main(args.reps, args.out)
