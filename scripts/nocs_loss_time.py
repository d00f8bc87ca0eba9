"""Time the NUNOCS symmetry-min cross-entropy loss (catgrasp_amd/loss.py) at the training configuration and write
profiles/nocs_loss_time.json:  python scripts/nocs_loss_time.py [--out FILE] [--reps R]

Workload: config_nunocs.yml, B = 34, N = 8192, bins = 100, for nut (12 symmetries) and screw (72), logits in both storages.
Per (category, storage), from HIP events around warm back-to-back calls (the median of --reps batches of CALLS calls each):
  forward_ms         the forward-only call of the validation loop (no lse kept), through the Python wrapper: its four torch.empty
                     calls and the gaps between its three launches are inside
  forward_train_ms   the forward that keeps lse for the backward, likewise
  forward_abi_ms     cg_nocs_symce_forward on buffers allocated once (no lse): the three launches alone
  backward_ms        the backward launch alone (cg_nocs_symce_backward on the saved lse and ids)
  step_ms            loss = crit(pred, target); loss.backward() through autograd, one call per event pair
and torch.cuda.max_memory_allocated above the inputs for the forward-only call and for the autograd step.  The script asserts that
the step allocates nothing above the gradient, lse, the workspace and the (B, S) outputs.

Share of HBM bandwidth = bytes the algorithm has to move / time / HBM_RATE, with the bytes stated here:
  forward    the logits once + the targets
  backward   the logits once + the gradient once + lse
HBM_RATE is 6.3e12 B/s, what a streaming float4 copy reaches on an MI355X (the data sheet says 8e12).  The copy rate of this run is
measured too: grad = pred.clone() of the same logits, 2 x the logits' bytes.

Baseline: the formula composed from torch operations on the same device (expand, cross_entropy per axis, sum, mean, argmin, gather),
which is what the reference module executes; its time, its peak memory and its loss are recorded next to ours.  It needs about
3 x B N bins S x 4 bytes (26 GB for screw); --no-baseline skips it."""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from catgrasp_amd import _lib as L  # noqa: E402
from catgrasp_amd import loss as nl  # noqa: E402
from catgrasp_amd._lib import _p, _stream, check  # noqa: E402

B, N, BINS = 34, 8192, 100
CALLS = 10
HBM_RATE = 6.3e12


def torch_composition(pred, target, tfs, bins):
    Bn, Nn = target.shape[:2]
    S = len(tfs)
    homo = torch.cat([target - 0.5, torch.ones_like(target[..., :1])], -1)
    moved = torch.matmul(tfs[None].expand(Bn, S, 4, 4), homo.permute(0, 2, 1)[:, None].expand(Bn, S, 4, Nn))
    moved = moved.permute(0, 1, 3, 2)[..., :3] + 0.5
    cls = torch.clamp(moved * bins, 0, bins - 1).long()
    x = pred.reshape(Bn, Nn, 3, bins)[..., None].expand(-1, -1, -1, -1, S)
    per_axis = [F.cross_entropy(x[:, :, a].permute(0, 2, 3, 1), cls[..., a], reduction='none') for a in range(3)]
    per_sym = torch.stack(per_axis, -1).sum(-1).mean(-1)
    ids = per_sym.argmin(1)
    return torch.gather(per_sym, 1, ids[:, None]).mean()


def timed(fn, reps, calls):
    """Median over `reps` batches of the device time of one of `calls` back-to-back calls, in ms."""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) / calls)
    return statistics.median(out), min(out), max(out)


def peak_above(fn):
    """Peak of torch's allocations during fn() above what was allocated before it, in bytes."""
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - before


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'nocs_loss_time.json'))
    ap.add_argument('--reps', type=int, default=9)
    ap.add_argument('--no-baseline', action='store_true')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('no HIP device: these are device timings, there is nothing to fall back to')
    dev = torch.device('cuda:0')
    torch.manual_seed(0)
    logits_bytes = B * N * 3 * BINS * 4
    res = {'device': torch.cuda.get_device_name(0), 'B': B, 'N': N, 'bins': BINS, 'reps': args.reps, 'calls_per_rep': CALLS,
           'hbm_rate_bytes_per_s': HBM_RATE, 'logits_bytes': logits_bytes, 'cases': {}}
    store = torch.randn(B, N, 3 * BINS, device=dev) * 3
    target = torch.rand(B, N, 3, device=dev)
    med, lo, hi = timed(lambda: store.clone(), args.reps, CALLS)
    res['clone'] = {'ms': med, 'ms_min': lo, 'ms_max': hi, 'bytes': 2 * logits_bytes, 'bytes_per_s': 2 * logits_bytes / (med * 1e-3)}
    for name in ('nut', 'screw'):
        crit = nl.NocsMinSymmetryCELoss({'nocs_class_name': name, 'ce_loss_bins': BINS})
        tfs = crit.symmetry_tfs(dev)
        S = crit.n_sym
        ws_bytes = 4 * int(L.lib().cg_nocs_symce_workspace_floats(B, N, BINS, S))
        lse_bytes, small = 4 * B * N * 3, 4 * (B * S + B + 1)
        fwd_bytes, bwd_bytes = logits_bytes + 4 * B * N * 3, 2 * logits_bytes + lse_bytes
        for storage in ('channel_major', 'point_major'):
            pred = store.permute(0, 2, 1).contiguous().permute(0, 2, 1) if storage == 'channel_major' else store
            layout = nl.layout_of(pred)
            case = {'S': S, 'forward_bytes': fwd_bytes, 'backward_bytes': bwd_bytes, 'workspace_bytes': ws_bytes, 'lse_bytes': lse_bytes}

            def forward_only():
                with torch.no_grad():
                    return crit(pred, target)
            for key, fn, nbytes in (('forward', forward_only, fwd_bytes),
                                    ('forward_train', lambda: nl._forward(pred, target, tfs, BINS, True), fwd_bytes + lse_bytes)):
                med, lo, hi = timed(fn, args.reps, CALLS)
                case.update({f'{key}_ms': med, f'{key}_ms_min': lo, f'{key}_ms_max': hi, f'{key}_hbm_share': nbytes / (med * 1e-3) / HBM_RATE})
            ws, out_loss, out_L = (torch.empty(n, dtype=torch.float32, device=dev) for n in (ws_bytes // 4, 1, B * S))
            out_ids = torch.empty(B, dtype=torch.int32, device=dev)

            def forward_abi():
                check(L.lib().cg_nocs_symce_forward(_p(pred), layout, _p(target), _p(tfs), B, N, BINS, S, _p(ws), _p(out_loss), _p(out_ids), _p(out_L),
                                                    None, _stream()), 'cg_nocs_symce_forward')
            med, lo, hi = timed(forward_abi, args.reps, CALLS)
            case.update({'forward_abi_ms': med, 'forward_abi_ms_min': lo, 'forward_abi_ms_max': hi, 'forward_abi_hbm_share': fwd_bytes / (med * 1e-3) / HBM_RATE})
            del ws, out_loss, out_L, out_ids
            _, ids, _, lse = nl._forward(pred, target, tfs, BINS, True)
            grad = torch.empty_strided(pred.shape, pred.stride(), dtype=torch.float32, device=dev)
            one = torch.ones((), device=dev)

            def backward():
                check(L.lib().cg_nocs_symce_backward(_p(pred), layout, _p(target), _p(tfs), _p(lse), _p(ids), _p(one), B, N, BINS, S, _p(grad),
                                                     _stream()), 'cg_nocs_symce_backward')
            med, lo, hi = timed(backward, args.reps, CALLS)
            case.update({'backward_ms': med, 'backward_ms_min': lo, 'backward_ms_max': hi, 'backward_hbm_share': bwd_bytes / (med * 1e-3) / HBM_RATE,
                         'backward_bytes_per_s': bwd_bytes / (med * 1e-3), 'backward_over_clone_rate': bwd_bytes / (med * 1e-3) / res['clone']['bytes_per_s']})
            del grad
            leaf = pred.detach().requires_grad_(True)

            def step():
                leaf.grad = None
                crit(leaf, target).backward()
            med, lo, hi = timed(step, args.reps, 1)
            case.update({'step_ms': med, 'step_ms_min': lo, 'step_ms_max': hi})
            leaf.grad = None
            case['forward_peak_bytes'] = peak_above(forward_only)
            case['step_peak_bytes'] = peak_above(step)
            allowed = logits_bytes + lse_bytes + ws_bytes + small + 64 * 1024       # gradient, lse, workspace, outputs; allocator rounding
            assert case['step_peak_bytes'] <= allowed, (case['step_peak_bytes'], allowed)
            assert case['forward_peak_bytes'] <= ws_bytes + small + 64 * 1024, case['forward_peak_bytes']
            case['loss'] = float(forward_only())
            leaf.grad = None
            del leaf
            if not args.no_baseline:
                base = pred.detach().requires_grad_(True)

                def base_forward():
                    with torch.no_grad():
                        return torch_composition(base, target, tfs, BINS)

                def base_step():
                    base.grad = None
                    torch_composition(base, target, tfs, BINS).backward()
                bl = {}
                try:
                    for key, fn in (('forward', base_forward), ('step', base_step)):
                        med, lo, hi = timed(fn, 3, 1)
                        bl.update({f'{key}_ms': med, f'{key}_ms_min': lo, f'{key}_ms_max': hi})
                    base.grad = None
                    bl['forward_peak_bytes'] = peak_above(base_forward)
                    bl['step_peak_bytes'] = peak_above(base_step)
                    bl['loss'] = float(base_forward())
                    assert abs(bl['loss'] - case['loss']) <= 1e-4 * max(1.0, abs(bl['loss'])), (bl['loss'], case['loss'])
                except torch.cuda.OutOfMemoryError as e:                 # recorded, not hidden: the expansion did not fit
                    bl['out_of_memory'] = str(e).splitlines()[0]
                base.grad = None
                del base
                case['torch_composition'] = bl
                torch.cuda.empty_cache()
            res['cases'][f'{name}_{storage}'] = case
            print(name, storage, json.dumps(case), flush=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write('\n')
    print('wrote', args.out)


if __name__ == '__main__':
    main()
