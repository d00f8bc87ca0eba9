"""CPU tests (no GPU) of the assembled PointGroup network: the yardstick tests/pointgroup_ref.py equals a dense float64 torch evaluation,
its test weights meet the condition the GPU bar rests on, the model has the reference's state_dict layout and loads its checkpoints,
the fourth header is plain C99 beside the other three and returns its error codes without a GPU, and the model refuses what it does
not run."""
import ctypes
import itertools
import json
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import catgrasp_amd.spconv as spconv
import pointgroup_ref as P
import sparse_ref as R
from catgrasp_amd import _lib, pointgroup

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
INCLUDE = os.path.dirname(_lib.POINTGROUP_HEADER_PATH)
HEADERS = ['catgrasp_amd.h', 'catgrasp_amd_cluster.h', 'catgrasp_amd_sparse.h', 'catgrasp_amd_pointgroup.h']


def _shipped_cfg():
    return pointgroup.config_from_yaml(os.path.join(GOLDEN, 'config_pointgroup.yaml'))


# ---- 1. the yardstick against a dense evaluation -------------------------------------------------------------------------------------

def _dense_unet(p, idx, x, shape, batch, planes):
    """input_conv and the U-Net on dense float64 grids: conv3d masked to the active sites, strided conv3d with outputs active where any
    input is, conv_transpose3d masked to the fine sites.  -> the rows of the active sites."""
    t = lambda key: torch.from_numpy(p[key].astype(np.float64))
    col = lambda v: v.view(1, -1, 1, 1, 1)
    mask = torch.from_numpy(R.dense(idx, np.ones((len(idx), 1)), batch, shape))

    def bn_relu(X, key, M):
        return ((X - col(t(key + '.running_mean'))) / torch.sqrt(col(t(key + '.running_var')) + P.EPS) * col(t(key + '.weight')) + col(t(key + '.bias'))).clamp(min=0) * M

    def subm(X, key, M):
        w = t(key + '.weight')
        return F.conv3d(X, w.permute(4, 3, 0, 1, 2), t(key + '.bias'), padding=w.shape[0] // 2) * M

    def block(X, key, cin, cout, M):
        h = subm(bn_relu(X, key + '.conv_branch.0', M), key + '.conv_branch.2', M)
        h = subm(bn_relu(h, key + '.conv_branch.3', M), key + '.conv_branch.5', M)
        return h + (X if cin == cout else subm(X, key + '.i_branch.0', M))

    def ublock(X, key, planes, M):
        n = planes[0]
        for i in range(2):
            X = block(X, f'{key}.blocks.block{i}', n, n, M)
        if len(planes) > 1:
            Mc = F.max_pool3d(M, 2, 2)                                                   # floor mode: the last site of an odd axis feeds nothing
            D = F.conv3d(bn_relu(X, key + '.conv.0', M), t(key + '.conv.2.weight').permute(4, 3, 0, 1, 2), t(key + '.conv.2.bias'), stride=2) * Mc
            D = ublock(D, key + '.u', planes[1:], Mc)
            up = F.conv_transpose3d(bn_relu(D, key + '.deconv.0', Mc), t(key + '.deconv.2.weight').permute(3, 4, 0, 1, 2), None, stride=2)
            pad = [v for s, u in zip(reversed(M.shape[2:]), reversed(up.shape[2:])) for v in (0, s - u)]
            U = (F.pad(up, pad) + col(t(key + '.deconv.2.bias'))) * M                    # a dropped site gets the bias only
            X = torch.cat([X, U], 1)
            X = block(X, key + '.blocks_tail.block0', 2 * n, n, M)
            X = block(X, key + '.blocks_tail.block1', n, n, M)
        return X

    X = subm(torch.from_numpy(R.dense(idx, x.astype(np.float64), batch, shape)), 'input_conv.0', mask)
    out = ublock(X, 'unet', planes, mask).numpy()
    return out[idx[:, 0], :, idx[:, 1], idx[:, 2], idx[:, 3]]


def test_the_yardstick_equals_a_dense_float64_evaluation():
    shape, batch, planes = (20, 16, 19), 2, [16, 32, 48]
    idx = R.scene(n=220, seed=11, batch=batch, shape=shape, special=False)
    lv = P.levels(idx, shape, depth=3)
    assert lv.dropped.any() and lv.down.dropped.any()                                    # both odd axes drop sites
    x = P.features(len(idx), seed=12)
    p = P.make_params(lv, x, planes=planes, seed=13)
    imap = P.point_map(len(idx), seed=14)
    feats, offsets = P.Net(p, planes=planes).forward(x, lv, imap)
    want = _dense_unet(p, idx, x, shape, batch, planes)
    assert np.abs(want).max() > 1 and np.abs(feats - want).max() <= 1e-10
    t = lambda key: torch.from_numpy(p[key].astype(np.float64))
    y = F.batch_norm(torch.from_numpy(want), t('output_layer.0.running_mean'), t('output_layer.0.running_var'), t('output_layer.0.weight'),
                     t('output_layer.0.bias'), False, 0.0, P.EPS).clamp(min=0)[torch.from_numpy(imap).long()]
    y = F.batch_norm(F.linear(y, t('offset.0.weight'), t('offset.0.bias')), t('offset.1.running_mean'), t('offset.1.running_var'), t('offset.1.weight'),
                     t('offset.1.bias'), False, 0.0, P.EPS).clamp(min=0)
    assert np.abs(offsets - F.linear(y, t('offset.3.weight'), t('offset.3.bias')).numpy()).max() <= 1e-10


def test_the_network_scenes_hold_every_trap():
    idx = P.scene('full')
    lv = P.scene_levels('full')
    sites = {tuple(r) for r in idx.tolist()}
    assert 590 <= len(idx) <= 610 and len(sites) == len(idx) and set(idx[:, 0]) == {0, 1}
    assert {(0, 0, 0, 0), (1, 149, 127, 130)} <= sites                                   # the two grid corners
    assert lv.dropped[idx[:, 3] == 130].all() and (idx[:, 3] == 130).sum() >= 2          # dropped by the first strided layer
    l2 = lv.down
    assert l2.shape == (75, 64, 65) and (l2.indices[:, 1] == 74).any()                   # dropped by the second: d0 in {148, 149}
    assert (l2.dropped == ((l2.indices[:, 1] == 74) | (l2.indices[:, 3] == 64))).all()
    octant = lambda r: (r[0], r[1] // 64, r[2] // 64, r[3] // 64)
    assert [octant(r) for r in idx.tolist()].count(octant(P.ISOLATED)) == 1              # alone in its 64^3 octant
    assert lv.counts()[-1] >= 4 and min(lv.counts()) >= 4
    assert P.scene_levels('n1').counts() == [1] * 7 and len(P.scene('n33')) == 33
    assert set(P.scene('item0_empty')[:, 0]) == {1}


# ---- 2. the condition on the test weights behind the GPU bar ------------------------------------------------------------------------

def test_float32_noise_of_the_test_weights_leaves_the_gpu_bar_a_factor_four():
    """A float32 evaluation of the same wiring (per-offset matrix products: not the kernel's summation order) is within
    2.5e-5 * max(1, |ref|) per element of the float64 one on every network scene, so the HIP path keeps a factor 4 below the suite's
    1e-4 for its own summation order.  A condition on the weight maker of tests/pointgroup_ref.py, not on the code under test.
    Measured: U-Net features 5.4e-6 / 3.4e-7 / 1.7e-7 / 1.8e-6 and pt_offsets 2.9e-6 / 2.9e-7 / 8.3e-8 / 7.4e-7 on full / n33 / n1 /
    item0_empty; max |ref| 14.0 (features) and 5.2 (offsets) on the full scene."""
    for kind in P.SCENES:
        f64, o64, _ = P.reference(kind)
        f32, o32, _ = P.reference(kind, 'float32')
        assert f32.dtype == np.float32 and o32.dtype == np.float32 and np.isfinite(f64).all()
        for name, got, ref in (('features', f32, f64), ('pt_offsets', o32, o64)):
            err = float(np.max(np.abs(got - ref) / np.maximum(1.0, np.abs(ref))))
            print(f'{kind} {name}: float32 error {err:.3g}, max |ref| {np.abs(ref).max():.3g}')
            assert err <= 2.5e-5, (kind, name, err)
    f64, o64, _ = P.reference('full')
    assert 0.5 < f64.std() < 5 and 0.2 < o64.std() < 5                                   # activations of order one at the end of the chain


# ---- 3. state_dict parity ----------------------------------------------------------------------------------------------------------

def test_state_dict_has_the_reference_keys_order_and_shapes():
    with open(os.path.join(GOLDEN, 'pointgroup_state_keys.json')) as f:
        want = json.load(f)
    assert len(want) == 583
    sd = pointgroup.PointGroup(_shipped_cfg()).state_dict()
    assert [[k, list(v.shape), str(v.dtype).replace('torch.', '')] for k, v in sd.items()] == want
    for key in ('unet.blocks_tail.block0.i_branch.0.weight', 'unet.u.conv.2.weight', 'offset.3.bias', 'score_linear.weight'):
        assert key in sd
    # the yardstick's parameters carry the same names and shapes
    shapes = {k: list(v.shape) for k, v in sd.items()}
    p = P.params()
    assert all(shapes[k] == list(v.shape) for k, v in p.items()) and len(p) == sum(not k.startswith('score_') and 'num_batches' not in k for k in sd)


def test_set_bn_init_and_module_tree():
    m = pointgroup.PointGroup(_shipped_cfg())
    bns = [mod for mod in m.modules() if isinstance(mod, torch.nn.BatchNorm1d)]
    assert len(bns) == 81 and all(bool((b.weight == 1).all()) and bool((b.bias == 0).all()) and b.eps == 1e-5 and b.momentum == 0.1 for b in bns)
    assert isinstance(m.unet.blocks.block0, pointgroup.ResidualBlock) and isinstance(m.unet.blocks.block0.i_branch[0], torch.nn.Identity)
    assert isinstance(m.unet.blocks_tail.block0.i_branch[0], spconv.SubMConv3d) and m.unet.u.u.u.u.u.u.nPlanes == [112]
    assert m.unet.conv[2].indice_key == 'spconv1' and m.unet.u.deconv[2].indice_key == 'spconv2' and m.unet.u.blocks.block1.conv_branch[5].indice_key == 'subm2'
    cfg = _shipped_cfg()
    cfg.block_residual = False
    vgg = pointgroup.PointGroup(cfg)
    assert isinstance(vgg.unet.blocks_tail.block0, pointgroup.VGGBlock) and vgg.unet.blocks_tail.block0.conv_layers[2].in_channels == 32
    cfg.m = 32                                                                           # 448 channels after the first skip: not built
    with pytest.raises(NotImplementedError):
        pointgroup.PointGroup(cfg)


def test_folded_batchnorm_constants_follow_the_tensors():
    """pointgroup._prologue keeps (scale, shift) per BatchNorm and remakes them after an in-place write, a load_state_dict or a
    replaced tensor; a write through .data moves no version counter and is seen only after model.eval() / .train()."""
    model = pointgroup.PointGroup(_shipped_cfg()).eval()
    bn = model.unet.conv[0]
    fold = lambda: tuple(t.clone() for t in pointgroup._prologue(bn))
    want = lambda: tuple(t.clone() for t in spconv.bn_relu_prologue(bn))
    same = lambda a, b: all(torch.equal(x, y) for x, y in zip(a, b))
    first = fold()
    assert same(first, want()) and pointgroup._prologue(bn)[0] is pointgroup._prologue(bn)[0]          # kept, not remade
    with torch.no_grad():
        bn.running_mean.add_(1.0)                                                          # in place
    second = fold()
    assert same(second, want()) and not same(second, first)
    sd = bn.state_dict()
    sd['running_var'] = sd['running_var'] * 4
    sd['weight'] = sd['weight'] * -0.5
    bn.load_state_dict(sd)
    third = fold()
    assert same(third, want()) and not same(third, second)
    bn.bias = torch.nn.Parameter(torch.full((16,), 0.25))                                  # replaced
    fourth = fold()
    assert same(fourth, want()) and not same(fourth, third)
    bn.weight.data.fill_(2.0)                                                              # through .data: the documented limit
    assert same(fold(), fourth) and not same(want(), fourth)
    model.eval()                                                                           # ... until the mode is set again
    assert same(fold(), want())
    bn.weight.data.fill_(3.0)
    model.train(); model.eval()
    assert same(fold(), want())


# ---- 4. checkpoints and configuration ----------------------------------------------------------------------------------------------

def test_load_model_follows_the_reference_rules(tmp_path):
    cfg = _shipped_cfg()
    torch.manual_seed(0)
    src = pointgroup.PointGroup(cfg)
    with torch.no_grad():
        src.unet.conv[0].running_mean.uniform_(-1, 1)
    ckpt = {'state_dict': {'module.' + k: v for k, v in src.state_dict().items()}, 'epoch': 3}
    torch.save(ckpt, tmp_path / 'best_val.pth.tar')
    dst = pointgroup.PointGroup(cfg)
    assert not torch.equal(dst.input_conv[0].weight, src.input_conv[0].weight)
    assert pointgroup.load_model(dst, str(tmp_path / 'best_val.pth.tar')) is dst
    for (k, a), (_, b) in zip(src.state_dict().items(), dst.state_dict().items()):
        assert torch.equal(a, b), k
    torch.save(src.state_dict(), tmp_path / 'bare.pth.tar')                              # a bare state dict loads too
    pointgroup.load_model(pointgroup.PointGroup(cfg), str(tmp_path / 'bare.pth.tar'))
    del ckpt['state_dict']['module.score_linear.weight']                                 # strict: the unused score branch must be there
    torch.save(ckpt, tmp_path / 'short.pth.tar')
    with pytest.raises(RuntimeError, match='score_linear.weight'):
        pointgroup.load_model(pointgroup.PointGroup(cfg), str(tmp_path / 'short.pth.tar'))


def test_config_from_yaml_flattens_the_sections():
    cfg = _shipped_cfg()
    assert cfg.m == 16 and cfg.use_coords is True and cfg.scale == 500 and cfg.full_scale == [128, 999999] and cfg.mode == 4
    assert cfg.block_residual is True and cfg.block_reps == 2 and cfg.input_channel == 3 and cfg.prepare_epochs == 999999
    assert cfg.downsample_size == 0.0005 and cfg.class_name == 'nut' and cfg.score_mode == 4 and not hasattr(cfg, 'GENERAL')


# ---- 5. the fourth header ------------------------------------------------------------------------------------------------------------

def test_pointgroup_header_is_strict_c99_in_any_order_and_links_from_c(tmp_path):
    if shutil.which('gcc') is None:
        pytest.fail('gcc is needed to check the header')
    syms = sorted(_lib.pointgroup_signatures())
    assert syms == ['cg_sparse_conv_cat']
    call = lambda a: f'cg_sparse_conv_cat({a})'
    body = ('#include <stdio.h>\ntypedef void (*fn_t)(void);\nint main(void) {\n  fn_t table[] = {\n' + ''.join(f'    (fn_t)&{s},\n' for s in syms) + '  };\n'
            '  int i[8] = {0}; float f[4] = {0};\n'
            '  int bad = 0;\n'
            f'  bad += {call("f, 8, f, 16, 1, i, 1, 27, f, f, f, f, f, 16, f, (void*)0")} != CG_ERR_UNSUPPORTED;      /* cin_a */\n'
            f'  bad += {call("f, 16, f, 24, 1, i, 1, 27, f, f, f, f, f, 16, f, (void*)0")} != CG_ERR_UNSUPPORTED;     /* cin_b */\n'
            f'  bad += {call("f, 128, f, 112, 1, i, 1, 27, f, f, f, f, f, 16, f, (void*)0")} != CG_ERR_UNSUPPORTED;   /* the sum */\n'
            f'  bad += {call("f, 16, f, 16, 1, i, 1, 27, f, f, f, f, f, 6, f, (void*)0")} != CG_ERR_UNSUPPORTED;      /* cout */\n'
            f'  bad += {call("f, 16, f, 16, 1, i, 1, 27, f, f, f, f, f, 128, f, (void*)0")} != CG_ERR_UNSUPPORTED;\n'
            f'  bad += {call("f, 16, f, 16, 1, i, 1, 9, f, f, f, f, f, 16, f, (void*)0")} != CG_ERR_ARG;              /* K */\n'
            f'  bad += {call("f, 16, f, 0, 1, i, 1, 27, f, f, f, f, f, 16, f, (void*)0")} != CG_ERR_ARG;              /* no second source */\n'
            f'  bad += {call("f, 16, (float*)0, 16, 1, i, 1, 27, f, f, f, f, f, 16, f, (void*)0")} != CG_ERR_ARG;     /* null feats_b */\n'
            f'  bad += {call("(float*)0, 16, f, 16, 1, i, 1, 27, f, f, f, f, f, 16, f, (void*)0")} != CG_ERR_ARG;\n'
            f'  bad += {call("f, 16, f, 16, 1, i, 1, 27, f, f, f, (float*)0, f, 16, f, (void*)0")} != CG_ERR_ARG;     /* scale without shift */\n'
            f'  bad += {call("f, 16, f, 16, 1, i, 1, 27, (float*)0, f, f, f, f, 16, f, (void*)0")} != CG_ERR_ARG;     /* null weight */\n'
            f'  bad += {call("f, 16, f, 16, 1, i, -1, 27, f, f, f, f, f, 16, f, (void*)0")} != CG_ERR_ARG;\n'
            f'  bad += {call("f, 16, f, 16, -1, i, 1, 27, f, f, f, f, f, 16, f, (void*)0")} != CG_ERR_ARG;\n'
            f'  bad += {call("f, 96, f, 96, 1, i, 0, 27, f, f, f, f, f, 3, f, (void*)0")} != CG_OK;                   /* no output rows */\n'
            '  printf("%d\\n", (int)(sizeof table / sizeof table[0]));\n'
            '  return bad;\n}\n')
    libdir = os.path.dirname(_lib.LIB_PATH)
    for n, order in enumerate(itertools.permutations(HEADERS)):
        # every order of inclusion, and the new header a second time
        src = ''.join(f'#include "{h}"\n' for h in order) + '#include "catgrasp_amd_pointgroup.h"\n' + body
        (tmp_path / f'main{n}.c').write_text(src)
        cmd = ['gcc', '-std=c99', '-Wall', '-Wextra', '-Werror', '-pedantic', '-I', INCLUDE, f'main{n}.c']
        if n:
            subprocess.check_call(cmd + ['-fsyntax-only'], cwd=tmp_path)
            continue
        subprocess.check_call(cmd + ['-L', libdir, '-lcatgrasp_amd', f'-Wl,-rpath,{libdir}', '-Wl,--allow-shlib-undefined', '-o', 'main'], cwd=tmp_path)
        out = subprocess.run([str(tmp_path / 'main')], capture_output=True, text=True)
        assert out.returncode == 0, (out.returncode, out.stderr)
        assert out.stdout.split() == ['1']
    (tmp_path / 'alone.c').write_text('#include "catgrasp_amd_pointgroup.h"\nint main(void) { return CG_OK; }\n')
    subprocess.check_call(['gcc', '-std=c99', '-Wall', '-Wextra', '-Werror', '-pedantic', '-I', INCLUDE, '-fsyntax-only', 'alone.c'], cwd=tmp_path)


def test_binding_takes_the_types_from_the_new_header_and_leaves_the_other_three_alone():
    lib = _lib.lib()
    vp, ci, cl = ctypes.c_void_p, ctypes.c_int, ctypes.c_long
    assert tuple(lib.cg_sparse_conv_cat.argtypes) == (vp, ci, vp, ci, cl, vp, cl, ci, vp, vp, vp, vp, vp, ci, vp, vp) and lib.cg_sparse_conv_cat.restype is ci
    with pytest.raises(ctypes.ArgumentError):
        lib.cg_sparse_conv_cat(None, 16.0, None, 16, 1, None, 1, 27, None, None, None, None, None, 16, None, None)
    assert lib.cg_sparse_conv_cat(None, 16, None, 16, 1, None, 1, 27, None, None, None, None, None, 16, None, None) == -1
    assert lib.cg_sparse_conv_cat(None, 16, None, 16, 1, None, 1, 27, None, None, None, None, None, 17, None, None) == -2
    assert len(_lib.declared_symbols()) == 71
    assert sorted(_lib.cluster_signatures()) == ['cg_meanshift_climb', 'cg_meanshift_lds_max_points', 'cg_meanshift_merge']
    assert sorted(_lib.sparse_signatures()) == ['cg_sparse_conv', 'cg_sparse_keys', 'cg_sparse_rules_down', 'cg_sparse_rules_inverse', 'cg_sparse_rules_subm']


def test_lib_raises_when_the_library_lacks_the_new_symbol(monkeypatch):
    real = _lib.pointgroup_signatures()
    monkeypatch.setattr(_lib, '_lib', None)
    monkeypatch.setattr(_lib, 'pointgroup_signatures', lambda: {**real, 'cg_pointgroup_not_built': (ctypes.c_int, ())})
    with pytest.raises(_lib.CatgraspAmdError, match='cg_pointgroup_not_built'):
        _lib.lib()


def test_sparse_conv_refuses_mismatched_sources():
    w = torch.zeros(27, 32, 16)
    nbr = torch.zeros(4, 27, dtype=torch.int32)
    with pytest.raises(ValueError, match='channels'):
        spconv.sparse_conv(torch.zeros(4, 16), nbr, w, features_b=torch.zeros(4, 32))
    with pytest.raises(ValueError, match='rows'):
        spconv.sparse_conv(torch.zeros(4, 16), nbr, w, features_b=torch.zeros(3, 16))


# ---- 6. refusals -----------------------------------------------------------------------------------------------------------------------

def test_forward_refusals(monkeypatch):
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)          # on a GPU host too: the refusal, not a CPU fallback
    model = pointgroup.PointGroup(_shipped_cfg())
    idx = torch.from_numpy(P.scene('n33'))
    x = spconv.SparseConvTensor(torch.zeros(len(idx), 6), idx, P.SHAPE, P.BATCH)
    imap = torch.arange(len(idx), dtype=torch.int32)
    args = (x, imap, None, None, None)
    with pytest.raises(NotImplementedError, match='eval'):
        model(*args, epoch=model.prepare_epochs - 1)                        # a fresh module is in training mode
    model.eval()
    with pytest.raises(NotImplementedError, match='score branch'):
        model(*args, epoch=model.prepare_epochs + 1)
    with pytest.raises(_lib.CatgraspAmdError):
        model(*args, epoch=model.prepare_epochs - 1)
    with pytest.raises(_lib.CatgraspAmdError):
        model.unet_features(x)
