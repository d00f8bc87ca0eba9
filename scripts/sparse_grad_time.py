"""dev: time of forward + backward of one sparse convolution layer (catgrasp_amd.spconv_autograd) -> profiles/sparse_grad_time.json.

  python scripts/sparse_grad_time.py          on the MI355X: HIP-event times, median of --reps (>= 20) after a warm-up

Cloud: the 11,914-voxel bin scene of scripts/sparse_conv_time.py, rows in random order and in key order.  Layers: SubMConv3d k = 3
at the widest level (224 -> 112) and at 16 -> 16, rule book built beforehand.  Timed per layer: forward + backward through the layer
class (input, weight and bias gradients), and its parts on their own: the forward launch, cg_sparse_conv_wgrad (both launches and
the workspace allocation), cg_sparse_conv_dgrad (with the weight permutation).  Beside it the only baseline there is -- the parent
commit has no backward: the same forward and gradients composed from torch ops on the device over the SAME rule book (per offset
index_select -> mm -> index_add, differentiated by autograd; the pair lists are made before the clock starts).  The script also
reports the largest difference between the two sets of gradients.

wgrad's share of the f32 MFMA peak: 2 * pairs * cin * cout (+ 2 * n * cout for the bias) FLOP over its time, against 157.3 TFLOP/s
(v_mfma_f32_32x32x2_f32, 64 FLOP per clock and SIMD at 2400 MHz).  The clocks `rocm-smi --showclocks` reports after the timed loops
are recorded as read."""
import argparse
import json
import os
import statistics
import subprocess
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, 'profiles', 'sparse_grad_time.json')
WIDTHS = ((224, 112), (16, 16))
PEAK_F32_MFMA = 157.3e12


def main(reps, out_path):
    import torch
    import catgrasp_amd.spconv_autograd as spconv
    from sparse_conv_time import bin_scene, voxels
    dev = torch.device('cuda:0')

    def timed(fn):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); out = fn(); b.record(); torch.cuda.synchronize()
            ms.append(a.elapsed_time(b))
        return round(statistics.median(ms), 4), out

    def measure(idx_np, shape):
        idx = torch.from_numpy(idx_np).to(dev)
        n = len(idx_np)
        book = spconv.subm_rules(idx, shape, 1)
        nbr = book.nbr
        plist = []
        for k in range(27):
            o = torch.nonzero(nbr[:, k] >= 0).flatten()
            if o.numel():
                plist.append((k, o, nbr[o, k].long()))
        pairs = int((nbr >= 0).sum())
        res = {'neighbours_per_site_of_27': round(pairs / n, 2), 'layers': []}
        g = torch.Generator(device='cpu').manual_seed(0)
        for cin, cout in WIDTHS:
            layer = spconv.SubMConv3d(cin, cout, 3, padding=1, indice_key='subm1').to(dev)
            with torch.no_grad():
                layer.weight.copy_(((torch.rand((3, 3, 3, cin, cout), generator=g) * 2 - 1) * (3.0 / cin) ** 0.5).to(dev))
            x = (torch.rand((n, cin), generator=g) * 2 - 1).to(dev).requires_grad_()
            dy = ((torch.rand((n, cout), generator=g) * 2 - 1) * (3.0 / n) ** 0.5).to(dev)
            w3 = layer.weight.detach().reshape(27, cin, cout)

            def hip_step():
                t = spconv.SparseConvTensor(x, idx, shape, 1)
                t.indice_dict['subm1'] = book
                x.grad = layer.weight.grad = layer.bias.grad = None
                layer(t).features.backward(dy)
                return layer.weight.grad.reshape(27, cin, cout), x.grad, layer.bias.grad

            wt = layer.weight.detach().reshape(27, cin, cout).clone().requires_grad_()
            bt = layer.bias.detach().clone().requires_grad_()

            def torch_step():
                x.grad = wt.grad = bt.grad = None
                out = torch.zeros((n, cout), dtype=torch.float32, device=dev)
                for k, o, i in plist:
                    out = out.index_add(0, o, torch.mm(x.index_select(0, i), wt[k]))
                (out + bt).backward(dy)
                return wt.grad, x.grad, bt.grad

            row = {'cin': cin, 'cout': cout}
            row['hip_forward_backward_ms'], got = timed(hip_step)
            got = [t.clone() for t in got]
            row['torch_ops_forward_backward_ms'], want = timed(torch_step)
            row['max_abs_difference_dw_dx_db'] = [float((a - b).abs().max()) for a, b in zip(got, want)]
            with torch.no_grad():
                xd = x.detach()
                row['hip_forward_ms'], _ = timed(lambda: spconv.sparse_conv(xd, nbr, w3, layer.bias.detach()))
                row['hip_wgrad_ms'], _ = timed(lambda: spconv.sparse_conv_wgrad(xd, nbr, dy, cin))
                row['hip_dgrad_ms'], _ = timed(lambda: spconv.sparse_conv_dgrad(dy, nbr, spconv.transposed_weight(w3, True)))
            flop = 2.0 * pairs * cin * cout + 2.0 * n * cout
            row['wgrad_flop'] = flop
            row['wgrad_tflops'] = round(flop / (row['hip_wgrad_ms'] * 1e-3) / 1e12, 3)
            row['wgrad_fraction_of_f32_mfma_peak'] = round(flop / (row['hip_wgrad_ms'] * 1e-3) / PEAK_F32_MFMA, 4)
            row['wgrad_workspace_mib'] = round(spconv.L.lib().cg_sparse_wgrad_workspace(n, 27, cin, cout) * 4 / 2 ** 20, 2)
            row['hip_faster_than_torch_ops'] = row['hip_forward_backward_ms'] < row['torch_ops_forward_backward_ms']
            res['layers'].append(row)
            print(row, flush=True)
        return res

    idx_np, shape = voxels(bin_scene())
    key = ((idx_np[:, 1].astype(np.int64) * shape[1]) + idx_np[:, 2]) * shape[2] + idx_np[:, 3]
    data = {'device': torch.cuda.get_device_name(0), 'reps': reps, 'timer': 'HIP events, median, three warm-up calls per shape', 'active_voxels': len(idx_np),
            'spatial_shape': shape, 'grad_rows_per_chunk': spconv.grad_rows(), 'f32_mfma_peak_tflops': PEAK_F32_MFMA / 1e12}
    data['rows_in_random_order'] = measure(idx_np, shape)
    data['rows_in_key_order'] = measure(idx_np[np.argsort(key)], shape)
    try:
        data['clocks_after_the_timed_loops'] = subprocess.run(['rocm-smi', '--showclocks'], capture_output=True, text=True, timeout=60).stdout.splitlines()
        data['clocks_after_the_timed_loops'] = [l.strip() for l in data['clocks_after_the_timed_loops'] if 'sclk' in l or 'mclk' in l]
    except Exception as e:          # the tool is not part of the product
        data['clocks_after_the_timed_loops'] = f'not read: {e}'
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, 'w') as f:
        json.dump({'catgrasp_amd_on_mi355x': data}, f, indent=1, sort_keys=True)
        f.write('\n')


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--out', default=OUT)
    args = ap.parse_args()
    main(args.reps, args.out)
