"""CPU tests (no GPU) of the sparse convolution layers' boundary: include/catgrasp_amd_sparse.h is plain C99 beside the other two
headers and links from C, argument errors come back without a GPU, the ctypes binding takes its types from the header and requires
its symbols, the Python layers refuse what is not built, carry the reference's state_dict layout, and refuse to run without a HIP
device."""
import ctypes
import itertools
import math
import os
import shutil
import subprocess
from collections import OrderedDict

import pytest
import torch
from torch import nn

import catgrasp_amd.spconv as spconv
from catgrasp_amd import _lib

INCLUDE = os.path.dirname(_lib.SPARSE_HEADER_PATH)
SPARSE_SYMBOLS = ['cg_sparse_conv', 'cg_sparse_keys', 'cg_sparse_rules_down', 'cg_sparse_rules_inverse', 'cg_sparse_rules_subm']
HEADERS = ['catgrasp_amd.h', 'catgrasp_amd_cluster.h', 'catgrasp_amd_sparse.h']


def test_sparse_header_is_strict_c99_in_any_order_and_links_from_c(tmp_path):
    if shutil.which('gcc') is None:
        pytest.fail('gcc is needed to check the header')
    syms = sorted(_lib.sparse_signatures())
    assert syms == SPARSE_SYMBOLS
    body = ('#include <stdio.h>\ntypedef void (*fn_t)(void);\nint main(void) {\n  fn_t table[] = {\n' + ''.join(f'    (fn_t)&{s},\n' for s in syms) + '  };\n'
            '  int i[8] = {0}; long long k[2] = {0, 1}; float f[4] = {0};\n'
            '  int bad = 0;\n'
            '  bad += cg_sparse_keys(i, -1, 2, 9, 12, 17, 0, k, i, (void*)0) != CG_ERR_ARG;                  /* n < 0 */\n'
            '  bad += cg_sparse_keys(i, 1, 0, 9, 12, 17, 0, k, i, (void*)0) != CG_ERR_ARG;                   /* batch_size */\n'
            '  bad += cg_sparse_keys(i, 1, 2, 0, 12, 17, 0, k, i, (void*)0) != CG_ERR_ARG;                   /* empty axis */\n'
            '  bad += cg_sparse_keys(i, 1, 2, 1, 12, 17, 1, k, i, (void*)0) != CG_ERR_ARG;                   /* axis below the kernel */\n'
            '  bad += cg_sparse_keys(i, 1, 2, 9, 12, 17, 2, k, i, (void*)0) != CG_ERR_ARG;                   /* coarse */\n'
            '  bad += cg_sparse_keys(i, 1, 2147483647, 2147483647, 2147483647, 17, 0, k, i, (void*)0) != CG_ERR_ARG;   /* keys overflow */\n'
            '  bad += cg_sparse_keys((int*)0, 1, 2, 9, 12, 17, 0, k, i, (void*)0) != CG_ERR_ARG;             /* null */\n'
            '  bad += cg_sparse_keys(i, 1, 2, 9, 12, 17, 0, k, (int*)0, (void*)0) != CG_ERR_ARG;\n'
            '  bad += cg_sparse_keys(i, 0, 2, 9, 12, 17, 0, k, i, (void*)0) != CG_OK;                        /* nothing to do */\n'
            '  bad += cg_sparse_rules_subm(i, k, k, 1, 9, 12, 17, (int*)0, i, (void*)0) != CG_ERR_ARG;\n'
            '  bad += cg_sparse_rules_subm(i, k, k, -1, 9, 12, 17, i, i, (void*)0) != CG_ERR_ARG;\n'
            '  bad += cg_sparse_rules_down(k, 2, k, k, 1, 9, 12, 17, i, i, i, (void*)0) != CG_ERR_ARG;        /* more outputs than inputs */\n'
            '  bad += cg_sparse_rules_down(k, 1, k, k, 1, 9, 1, 17, i, i, i, (void*)0) != CG_ERR_ARG;\n'
            '  bad += cg_sparse_rules_down((long long*)0, 1, k, k, 1, 9, 12, 17, i, i, i, (void*)0) != CG_ERR_ARG;\n'
            '  bad += cg_sparse_rules_inverse(i, 1, k, 1, 9, 12, 17, (int*)0, (void*)0) != CG_ERR_ARG;\n'
            '  bad += cg_sparse_rules_inverse(i, -1, k, 1, 9, 12, 17, i, (void*)0) != CG_ERR_ARG;\n'
            '  bad += cg_sparse_conv(f, 1, i, 1, 27, f, f, f, f, f, 17, 16, f, (void*)0) != CG_ERR_UNSUPPORTED;    /* cin */\n'
            '  bad += cg_sparse_conv(f, 1, i, 1, 27, f, f, f, f, f, 240, 16, f, (void*)0) != CG_ERR_UNSUPPORTED;\n'
            '  bad += cg_sparse_conv(f, 1, i, 1, 27, f, f, f, f, f, 16, 128, f, (void*)0) != CG_ERR_UNSUPPORTED;   /* cout */\n'
            '  bad += cg_sparse_conv(f, 1, i, 1, 27, f, f, f, f, f, 16, 6, f, (void*)0) != CG_ERR_UNSUPPORTED;\n'
            '  bad += cg_sparse_conv(f, 1, i, 1, 9, f, f, f, f, f, 16, 16, f, (void*)0) != CG_ERR_ARG;             /* K */\n'
            '  bad += cg_sparse_conv(f, 1, i, 1, 27, f, f, f, (float*)0, f, 16, 16, f, (void*)0) != CG_ERR_ARG;    /* scale without shift */\n'
            '  bad += cg_sparse_conv(f, 1, i, 1, 27, (float*)0, f, f, f, f, 16, 16, f, (void*)0) != CG_ERR_ARG;    /* null weight */\n'
            '  bad += cg_sparse_conv(f, 1, i, -1, 27, f, f, f, f, f, 16, 16, f, (void*)0) != CG_ERR_ARG;\n'
            '  bad += cg_sparse_conv(f, 1, i, 0, 27, f, f, f, f, f, 6, 3, f, (void*)0) != CG_OK;                   /* no output rows */\n'
            '  printf("%d %d %d\\n", (int)(sizeof table / sizeof table[0]), CG_SPARSE_MAX_CIN, CG_SPARSE_MAX_COUT);\n'
            '  return bad;\n}\n')
    libdir = os.path.dirname(_lib.LIB_PATH)
    for n, order in enumerate(itertools.permutations(HEADERS)):
        # every order of inclusion, and the sparse header a second time
        src = ''.join(f'#include "{h}"\n' for h in order) + '#include "catgrasp_amd_sparse.h"\n' + body
        (tmp_path / f'main{n}.c').write_text(src)
        cmd = ['gcc', '-std=c99', '-Wall', '-Wextra', '-Werror', '-pedantic', '-I', INCLUDE, f'main{n}.c']
        if n:
            subprocess.check_call(cmd + ['-fsyntax-only'], cwd=tmp_path)
            continue
        subprocess.check_call(cmd + ['-L', libdir, '-lcatgrasp_amd', f'-Wl,-rpath,{libdir}', '-Wl,--allow-shlib-undefined', '-o', 'main'], cwd=tmp_path)
        out = subprocess.run([str(tmp_path / 'main')], capture_output=True, text=True)
        assert out.returncode == 0, (out.returncode, out.stderr)
        assert out.stdout.split() == [str(len(syms)), str(spconv.MAX_CIN), str(spconv.MAX_COUT)]
    # the sparse header alone
    (tmp_path / 'alone.c').write_text('#include "catgrasp_amd_sparse.h"\nint main(void) { return CG_OK; }\n')
    subprocess.check_call(['gcc', '-std=c99', '-Wall', '-Wextra', '-Werror', '-pedantic', '-I', INCLUDE, '-fsyntax-only', 'alone.c'], cwd=tmp_path)


def test_binding_takes_the_sparse_types_from_the_header():
    lib = _lib.lib()
    vp, ci, cl = ctypes.c_void_p, ctypes.c_int, ctypes.c_long
    assert tuple(lib.cg_sparse_keys.argtypes) == (vp, cl, ci, ci, ci, ci, ci, vp, vp, vp)
    assert tuple(lib.cg_sparse_rules_subm.argtypes) == (vp, vp, vp, cl, ci, ci, ci, vp, vp, vp)
    assert tuple(lib.cg_sparse_rules_down.argtypes) == (vp, cl, vp, vp, cl, ci, ci, ci, vp, vp, vp, vp)
    assert tuple(lib.cg_sparse_rules_inverse.argtypes) == (vp, cl, vp, cl, ci, ci, ci, vp, vp)
    assert tuple(lib.cg_sparse_conv.argtypes) == (vp, cl, vp, cl, ci, vp, vp, vp, vp, vp, ci, ci, vp, vp)
    for name in SPARSE_SYMBOLS:
        assert getattr(lib, name).restype is ci
    with pytest.raises(ctypes.ArgumentError):
        lib.cg_sparse_conv(None, 1, None, 1, 27.0, None, None, None, None, None, 16, 16, None, None)      # a float for K never reaches C
    assert lib.cg_sparse_conv(None, 1, None, 1, 27, None, None, None, None, None, 16, 16, None, None) == -1
    assert lib.cg_sparse_conv(None, 1, None, 1, 27, None, None, None, None, None, 16, 17, None, None) == -2
    # the other headers' views are unchanged
    assert not set(SPARSE_SYMBOLS) & (set(_lib.declared_symbols()) | set(_lib.cluster_signatures()))


def test_lib_raises_when_the_library_lacks_a_sparse_symbol(monkeypatch):
    real = _lib.sparse_signatures()
    monkeypatch.setattr(_lib, '_lib', None)
    monkeypatch.setattr(_lib, 'sparse_signatures', lambda: {**real, 'cg_sparse_not_built': (ctypes.c_int, ())})
    with pytest.raises(_lib.CatgraspAmdError, match='cg_sparse_not_built'):
        _lib.lib()


def test_constructor_refusals():
    for make in (lambda: spconv.SubMConv3d(16, 16, 5, padding=2), lambda: spconv.SubMConv3d(16, 16, 2), lambda: spconv.SubMConv3d(16, 16, 3),
                 lambda: spconv.SubMConv3d(16, 16, 3, padding=1, dilation=2), lambda: spconv.SubMConv3d(16, 16, 3, padding=1, groups=2),
                 lambda: spconv.SparseConv3d(16, 32, 3, stride=2), lambda: spconv.SparseConv3d(16, 32, 2, stride=1),
                 lambda: spconv.SparseConv3d(16, 32, 2, stride=2, padding=1), lambda: spconv.SparseConv3d(16, 32, 3, stride=2, padding=1),
                 lambda: spconv.SparseInverseConv3d(32, 16, 3, indice_key='spconv1')):
        with pytest.raises(NotImplementedError):
            make()
    for cin, cout in ((7, 16), (8, 16), (240, 16), (0, 16), (16, 6), (16, 8), (16, 128), (16, 0)):
        with pytest.raises(ValueError):
            spconv.SubMConv3d(cin, cout, 3, padding=1)
    with pytest.raises(ValueError):
        spconv.SparseInverseConv3d(32, 16, 2, indice_key=None)
    # what the reference network constructs (pointgroup.py)
    spconv.SubMConv3d(6, 16, kernel_size=3, padding=1, bias=True, indice_key='subm1')
    spconv.SubMConv3d(32, 16, kernel_size=1, bias=True)
    spconv.SparseConv3d(16, 32, kernel_size=2, stride=2, bias=True, indice_key='spconv1')
    spconv.SparseInverseConv3d(32, 16, kernel_size=2, bias=True, indice_key='spconv1')
    spconv.SubMConv3d(224, 112, 3, padding=1)
    spconv.SubMConv3d(16, 3, 3, padding=1)
    with pytest.raises(ValueError):
        spconv.SparseConvTensor(torch.zeros(3, 6), torch.zeros(4, 4, dtype=torch.int32), [9, 12, 17], 2)        # mismatched rows
    with pytest.raises(ValueError):
        spconv.SparseConvTensor(torch.zeros(3, 6), torch.zeros(3, 3, dtype=torch.int32), [9, 12, 17], 2)
    with pytest.raises(ValueError):
        spconv.SparseConvTensor(torch.zeros(3, 6), torch.zeros(3, 4, dtype=torch.int32), [9, 12], 2)


def test_state_dict_keys_shapes_and_initialisation_follow_the_reference_layout():
    torch.manual_seed(0)
    cases = [(spconv.SubMConv3d(32, 16, 3, padding=1, indice_key='subm1'), (3, 3, 3, 32, 16)),
             (spconv.SubMConv3d(32, 16, 1), (1, 1, 1, 32, 16)),
             (spconv.SparseConv3d(16, 32, 2, stride=2, indice_key='spconv1'), (2, 2, 2, 16, 32)),
             (spconv.SparseInverseConv3d(32, 16, 2, indice_key='spconv1'), (2, 2, 2, 32, 16))]
    for layer, shape in cases:
        sd = layer.state_dict()
        assert list(sd) == ['weight', 'bias'] and tuple(sd['weight'].shape) == shape and tuple(sd['bias'].shape) == (shape[-1],)
        assert sd['weight'].dtype == torch.float32 and isinstance(layer, spconv.SparseModule)
        # kaiming_uniform_(a = sqrt(5)) as torch computes the fan of this layout: bound = sqrt(6 / (6 * fan)) with fan = shape[1] * prod(shape[2:])
        wb = 1 / math.sqrt(shape[1] * math.prod(shape[2:]))
        bb = 1 / math.sqrt(shape[3] * math.prod(shape[:3]))
        w, b = sd['weight'], sd['bias']
        assert w.abs().max() <= wb and w.abs().max() > 0.9 * wb and abs(float(w.mean())) < 0.1 * wb
        assert b.abs().max() <= bb and b.abs().max() > 0.5 * bb
    nb = spconv.SubMConv3d(16, 16, 3, padding=1, bias=False)
    assert list(nb.state_dict()) == ['weight'] and nb.bias is None
    # a block wired like the reference's loads a state dict with the reference's key names
    seq = spconv.SparseSequential(nn.BatchNorm1d(16), nn.ReLU(), spconv.SubMConv3d(16, 16, 3, padding=1, indice_key='subm1'))
    assert [k for k in seq.state_dict() if not k.startswith('0.')] == ['2.weight', '2.bias'] and len(seq) == 3
    named = spconv.SparseSequential(OrderedDict([('block0', spconv.SubMConv3d(16, 16, 1)), ('block1', nn.Identity())]))
    assert list(named.state_dict()) == ['block0.weight', 'block0.bias'] and isinstance(named[1], nn.Identity) and isinstance(named[-2], spconv.SubMConv3d)
    kw = spconv.SparseSequential(conv1=spconv.SubMConv3d(16, 16, 1), relu1=nn.ReLU())
    assert list(kw.state_dict()) == ['conv1.weight', 'conv1.bias']
    with pytest.raises(ValueError):
        spconv.SparseSequential(nn.ReLU(), **{'0': nn.ReLU()})


def test_forward_without_a_hip_device_raises(monkeypatch):
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)          # on a GPU host too: the refusal, not a CPU fallback
    x = spconv.SparseConvTensor(torch.zeros(3, 16), torch.tensor([[0, 0, 0, 0], [0, 1, 1, 1], [1, 2, 2, 2]], dtype=torch.int32), [9, 12, 17], 2)
    assert x.find_indice_pair('subm1') is None and x.find_indice_pair(None) is None and x.indice_dict == {}
    assert tuple(x.dense().shape) == (2, 16, 9, 12, 17) and tuple(x.dense(channels_first=False).shape) == (2, 9, 12, 17, 16)
    layers = [spconv.SubMConv3d(16, 16, 3, padding=1), spconv.SubMConv3d(16, 16, 1), spconv.SparseConv3d(16, 32, 2, stride=2, indice_key='k'),
              spconv.SparseSequential(nn.BatchNorm1d(16), nn.ReLU(), spconv.SubMConv3d(16, 16, 3, padding=1)).eval()]
    for layer in layers:
        with torch.no_grad(), pytest.raises((_lib.CatgraspAmdError, NotImplementedError)):
            layer(x)


def test_replace_feature_shares_the_bookkeeping():
    idx = torch.tensor([[0, 0, 0, 0], [0, 1, 1, 1], [1, 2, 2, 2]], dtype=torch.int32)
    x = spconv.SparseConvTensor(torch.zeros(3, 16), idx, [9, 12, 17], 2, grid=object())
    x.indice_dict['subm1'] = 'a rule book'
    feats = torch.ones(3, 32)
    y = x.replace_feature(feats)                                            # the same sites by default
    assert y is not x and y.features is feats and x.features.shape == (3, 16)
    assert y.indice_dict is x.indice_dict and y.grid is x.grid
    assert y.indices is x.indices and y.spatial_shape == [9, 12, 17] and y.batch_size == 2
    y.indice_dict['spconv1'] = 'another'                                    # a book built below is seen above
    assert x.find_indice_pair('spconv1') == 'another'
    out_idx, out_feats = torch.tensor([[0, 0, 0, 0], [1, 1, 1, 1]], dtype=torch.int32), torch.ones(2, 48)
    z = x.replace_feature(out_feats, out_idx, (4, 6, 8))                    # a layer whose output sites differ
    assert z.features is out_feats and z.indices is out_idx and z.spatial_shape == [4, 6, 8] and z.batch_size == 2
    assert z.indice_dict is x.indice_dict and z.grid is x.grid
    with pytest.raises(ValueError, match='rows'):
        x.replace_feature(torch.ones(2, 16))


@pytest.mark.parametrize('n', [0, 1, 5])
def test_identity_rules_is_the_arange_column(n):
    rows = spconv.identity_rules(n, torch.device('cpu'))
    want = torch.arange(n, dtype=torch.int32, device=torch.device('cpu')).view(n, 1)
    assert rows.dtype == torch.int32 and tuple(rows.shape) == (n, 1) and rows.device == want.device and torch.equal(rows, want)
