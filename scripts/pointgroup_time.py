"""dev: time of the assembled PointGroup network (catgrasp_amd.pointgroup) at the shipped configuration -> profiles/pointgroup_time.json.

  python scripts/pointgroup_time.py          on the MI355X: HIP-event times, median of --reps after a warm-up

Cloud: the 11,914-voxel bin scene of scripts/sparse_conv_time.py (16,384 points at 500 voxels per metre), rows in random order.
Weights: the constructor's initialisation (times do not depend on values).

Timed:
  the whole eval forward on the fused launches, and its parts: the 19 rule-book builds, the 71 U-Net launches over ready rule books,
  the head (2 launches and the row gather);
  the same network wired the plain way -- SparseSequential, torch.cat, +=, written out below -- whole and over ready rule books;
  for n in 16 .. 96, on the level-1 rule book, what the two-source kernel replaces in the first block after a skip: cg_sparse_conv_cat
  n+n -> n with K = 27 (prologue) and K = 1, against torch.cat + cg_sparse_conv on the concatenated matrix."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.join(HERE, '..')
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
from sparse_conv_time import bin_scene, voxels  # noqa: E402

OUT = os.path.join(ROOT, 'profiles', 'pointgroup_time.json')
SHIPPED = dict(input_channel=3, m=16, block_reps=2, block_residual=True, use_coords=True, cluster_radius=0.001, cluster_radius_shift=0.0005,
               cluster_meanActive=50, cluster_shift_meanActive=100, cluster_npoint_thre=200, score_fullscale=14, score_mode=4, prepare_epochs=999999,
               pretrain_module=[], fix_module=[], scale=500, mode=4)


def main(reps, out_path):
    import torch
    import catgrasp_amd.spconv as spconv
    from catgrasp_amd import pointgroup
    dev = torch.device('cuda:0')

    def timed(fn):
        fn(); torch.cuda.synchronize()
        ms = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); out = fn(); b.record(); torch.cuda.synchronize()
            ms.append(a.elapsed_time(b))
        return round(statistics.median(ms), 4), out

    torch.manual_seed(0)
    model = pointgroup.PointGroup(argparse.Namespace(**SHIPPED)).to(dev).eval()
    idx_np, shape = voxels(bin_scene())
    idx = torch.from_numpy(idx_np).to(dev)
    n = len(idx_np)
    feats = (torch.rand((n, 6), generator=torch.Generator().manual_seed(1)) * 2 - 1).to(dev)
    imap = torch.randint(n, (16384,), generator=torch.Generator().manual_seed(2)).int().to(dev)
    books = {}

    def tensor(ready):
        x = spconv.SparseConvTensor(feats, idx, shape, 1)
        if ready:
            x.indice_dict = books
        return x

    def rule_books():
        ind, shp = idx, shape
        for level in range(1, 8):
            spconv.subm_rules(ind, shp, 1)
            if level < 7:
                down = spconv.down_rules(ind, shp, 1)
                spconv.inverse_rules(down)
                ind, shp = down.out_indices, down.out_spatial_shape

    # the same modules wired the plain way: SparseSequential (BatchNorm + ReLU folded into the next layer), torch.cat, +=
    def plain_block(block, x):
        identity = spconv.SparseConvTensor(x.features, x.indices, x.spatial_shape, x.batch_size)
        out = block.conv_branch(x)
        out.features += block.i_branch(identity).features
        return out

    def plain_ublock(u, x):
        for block in u.blocks:
            x = plain_block(block, x)
        if len(u.nPlanes) > 1:
            decoder = u.deconv(plain_ublock(u.u, u.conv(x)))
            x.features = torch.cat((x.features, decoder.features), dim=1)
            for block in u.blocks_tail:
                x = plain_block(block, x)
        return x

    def plain_unet(ready):
        return plain_ublock(model.unet, model.input_conv(tensor(ready)))

    def plain(ready):
        return model.offset(model.output_layer(plain_unet(ready)).features[imap.long()])

    data = {'device': torch.cuda.get_device_name(0), 'reps': reps, 'active_voxels': n, 'points': int(imap.shape[0]), 'spatial_shape': shape,
            'timer': 'HIP events around the python calls, median; a forward is launch-bound, so the times include the host side of every launch',
            'two_source_kernel_in_forward': pointgroup.USE_TWO_SOURCE_KERNEL}
    with torch.no_grad():
        first = tensor(False)
        unet = model.unet_features(first)
        books.update(first.indice_dict)
        data['voxels_per_level'] = [int(books[f'subm{i}'].in_indices.shape[0]) for i in range(1, 8)]
        data['fused_forward_ms'], ret = timed(lambda: model(tensor(False), imap, None, None, None, epoch=0))
        data['rule_books_ms'], _ = timed(rule_books)
        data['fused_unet_launches_ms'], _ = timed(lambda: model.unet_features(tensor(True)))
        shipped = pointgroup.USE_TWO_SOURCE_KERNEL
        for flag, name in ((True, 'two_source'), (False, 'torch_cat')):           # the 71 launches with either form of the six skips
            pointgroup.USE_TWO_SOURCE_KERNEL = flag
            data[f'fused_unet_launches_{name}_skips_ms'], _ = timed(lambda: model.unet_features(tensor(True)))
        pointgroup.USE_TWO_SOURCE_KERNEL = shipped
        data['head_ms'], _ = timed(lambda: model.head(unet.features)[imap.long()])
        data['plain_forward_ms'], want = timed(lambda: plain(False))
        data['plain_forward_ready_rule_books_ms'], _ = timed(lambda: plain(True))
        data['fused_equals_plain_unet_bits'] = bool(torch.equal(plain_unet(True).features, unet.features))
        data['fused_vs_plain_offsets_max_abs_difference'] = float((ret['pt_offsets'] - want).abs().max())

        nbr = books['subm1'].nbr
        own = torch.arange(n, dtype=torch.int32, device=dev).view(n, 1)
        g = torch.Generator().manual_seed(3)
        rows = []
        for w_ in (16, 32, 48, 64, 80, 96):
            rnd = lambda *s: (torch.rand(s, generator=g) * 2 - 1).to(dev)
            a, b = rnd(n, w_), rnd(n, w_)
            w27, w1, bias = rnd(27, 2 * w_, w_) * (3.0 / (2 * w_)) ** 0.5, rnd(1, 2 * w_, w_), rnd(w_)
            scale, shift = rnd(2 * w_), rnd(2 * w_)
            row = {'n': w_}
            row['two_source_k27_ms'], t27 = timed(lambda: spconv.sparse_conv(a, nbr, w27, bias, scale, shift, features_b=b))
            row['two_source_k1_ms'], t1 = timed(lambda: spconv.sparse_conv(a, own, w1, bias, features_b=b))
            row['torch_cat_ms'], cat = timed(lambda: torch.cat((a, b), 1))
            row['one_source_k27_ms'], o27 = timed(lambda: spconv.sparse_conv(cat, nbr, w27, bias, scale, shift))
            row['one_source_k1_ms'], o1 = timed(lambda: spconv.sparse_conv(cat, own, w1, bias))

            def replaced():
                c = torch.cat((a, b), 1)
                return spconv.sparse_conv(c, nbr, w27, bias, scale, shift), spconv.sparse_conv(c, own, w1, bias)
            row['two_source_pair_ms'], _ = timed(lambda: (spconv.sparse_conv(a, nbr, w27, bias, scale, shift, features_b=b),
                                                          spconv.sparse_conv(a, own, w1, bias, features_b=b)))
            row['replaced_sequence_ms'], _ = timed(replaced)
            row['same_bits'] = bool(torch.equal(t27, o27) and torch.equal(t1, o1))
            rows.append(row)
            print(row, flush=True)
        data['skip_block_n_plus_n_to_n'] = rows
    print({k: v for k, v in data.items() if k != 'skip_block_n_plus_n_to_n'}, flush=True)
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
