"""CPU tests (no GPU) of the boundary of the batch-statistics BatchNorm + ReLU: include/catgrasp_amd_bn.h is plain C99, alone and next to
the other eight headers in either order, and links from C; every argument error comes back without a GPU; the workspace size is a
function of the shapes; the ctypes binding takes its types from that header and lib() requires its symbols; the build tracks it; the
Python wrapper refuses what it does not build before any device work."""
import ctypes
import inspect
import os
import re
import shutil
import subprocess

import pytest
import torch
from torch import nn

from catgrasp_amd import _lib, batchnorm

INCLUDE = os.path.dirname(_lib.BN_HEADER_PATH)
BN_SYMBOLS = ['cg_bn_relu_train_backward', 'cg_bn_relu_train_forward', 'cg_bn_workspace']
HEADERS = ['catgrasp_amd.h', 'catgrasp_amd_cluster.h', 'catgrasp_amd_sparse.h', 'catgrasp_amd_pointgroup.h', 'catgrasp_amd_scene.h',
           'catgrasp_amd_neighbors.h', 'catgrasp_amd_kdtree.h', 'catgrasp_amd_sparse_grad.h', 'catgrasp_amd_bn.h']
GCC = ['gcc', '-std=c99', '-Wall', '-Wextra', '-Werror', '-pedantic', '-I', INCLUDE]


def test_bn_header_is_strict_c99_alone_and_with_the_others_and_links_from_c(tmp_path):
    if shutil.which('gcc') is None:
        pytest.fail('gcc is needed to check the header')
    assert sorted(_lib.bn_signatures()) == BN_SYMBOLS
    fwd = 'cg_bn_relu_train_forward({x}, {n}, {c}, {gamma}, {beta}, 1e-5f, {ws}, {mean}, f, f, f, f, {y}, (void*)0)'
    bwd = 'cg_bn_relu_train_backward({x}, {dy}, {n}, {c}, {mean}, f, f, f, {ws}, {dgamma}, f, {dx}, (void*)0)'
    good = dict(x='f', n='4L', c='16', gamma='f', beta='f', ws='f', mean='f', y='f', dy='f', dgamma='f', dx='f')
    # the host array stands in for device memory: nothing may be launched, so nothing reads it
    null = '(float*)0'
    cases = [(fwd, b, 'CG_ERR_ARG') for b in (dict(x=null), dict(gamma=null), dict(beta=null), dict(ws=null), dict(mean=null), dict(y=null),
                                              dict(n='1L'), dict(n='0L'), dict(n='-1L'), dict(n='16777217L'), dict(c='0'), dict(c='-16'))]
    cases += [(bwd, b, 'CG_ERR_ARG') for b in (dict(x=null), dict(dy=null), dict(mean=null), dict(ws=null), dict(dgamma=null), dict(n='1L'),
                                              dict(n='16777217L'), dict(c='0'))]
    for call in (fwd, bwd):
        cases += [(call, dict(c=c), 'CG_ERR_UNSUPPORTED') for c in ('8', '240', '17', '6')]
        cases += [(call, dict(n='1L', c='8'), 'CG_ERR_ARG')]                                  # the count is judged before the width
    body = ''.join(f'  bad += {call.format(**{**good, **b})} != {want};   /* {b} */\n' for call, b, want in cases)
    for n, c, want in ((2, 16, 32), (1024, 16, 32), (1025, 16, 64), (2049, 112, 2 * 112 * 3), (16777216, 224, 2 * 224 * 16384)):
        body += f'  bad += cg_bn_workspace({n}L, {c}) != {want}L;\n'
    body += ('  bad += cg_bn_workspace(5L, 8) != CG_ERR_UNSUPPORTED;\n  bad += cg_bn_workspace(5L, 240) != CG_ERR_UNSUPPORTED;\n'
             '  bad += cg_bn_workspace(1L, 16) != CG_ERR_ARG;\n  bad += cg_bn_workspace(16777217L, 16) != CG_ERR_ARG;\n')
    for k, order in enumerate((HEADERS, HEADERS[::-1])):
        src = (''.join(f'#include "{h}"\n' for h in order) + '#include "catgrasp_amd_bn.h"\n#include <stdio.h>\n'
               'typedef void (*fn_t)(void);\nint main(void) {\n  fn_t table[] = {\n' + ''.join(f'    (fn_t)&{s},\n' for s in BN_SYMBOLS)
               + '  };\n  float f[4];\n  int bad = 0;\n  f[0] = 0.f;\n' + body
               + '  printf("%d %d %d\\n", (int)(sizeof table / sizeof table[0]), CG_BN_SEG, CG_BN_ROWS);\n  return bad;\n}\n')
        (tmp_path / f'main{k}.c').write_text(src)
        libdir = os.path.dirname(_lib.LIB_PATH)
        subprocess.check_call(GCC + [f'main{k}.c', '-L', libdir, '-lcatgrasp_amd', f'-Wl,-rpath,{libdir}', '-Wl,--allow-shlib-undefined', '-o', f'main{k}'],
                              cwd=tmp_path)
        out = subprocess.run([str(tmp_path / f'main{k}')], capture_output=True, text=True)
        assert out.returncode == 0, (out.returncode, out.stdout, out.stderr)
        assert out.stdout.split() == ['3', '64', '1024']
    (tmp_path / 'alone.c').write_text('#include "catgrasp_amd_bn.h"\nint main(void) { return CG_OK; }\n')
    subprocess.check_call(GCC + ['-fsyntax-only', 'alone.c'], cwd=tmp_path)


def test_binding_takes_the_bn_types_from_the_header_and_leaves_the_other_headers_alone():
    lib = _lib.lib()
    vp, ci, cl, cf = ctypes.c_void_p, ctypes.c_int, ctypes.c_long, ctypes.c_float
    scalar = {'int': ci, 'long': cl, 'float': cf}
    with open(_lib.BN_HEADER_PATH) as f:
        text = re.sub(r'/\*.*?\*/', '', f.read(), flags=re.S)
    for name in BN_SYMBOLS:
        m = re.search(r'\b(int|long)\s+' + name + r'\s*\(([^)]*)\)\s*;', text)
        params = [' '.join(q.split()) for q in m.group(2).split(',')]
        fn = getattr(lib, name)
        assert fn.restype is scalar[m.group(1)] and len(fn.argtypes) == len(params), name
        for at, q in zip(fn.argtypes, params):
            assert at is (vp if '*' in q else scalar[q.rsplit(' ', 1)[0]]), (name, q)
    assert tuple(lib.cg_bn_workspace.argtypes) == (cl, ci) and lib.cg_bn_workspace.restype is cl
    assert tuple(lib.cg_bn_relu_train_forward.argtypes) == (vp, cl, ci, vp, vp, cf) + (vp,) * 8
    assert tuple(lib.cg_bn_relu_train_backward.argtypes) == (vp, vp, cl, ci) + (vp,) * 9
    with pytest.raises(ctypes.ArgumentError):
        lib.cg_bn_workspace(5, 16.0)                                                         # a float for c never reaches C
    assert [lib.cg_bn_workspace(n, 16) for n in (2, 1024, 1025, 2049)] == [32, 32, 64, 96]
    assert lib.cg_bn_workspace(2 ** 24, 224) == 2 * 224 * 2 ** 14
    assert [lib.cg_bn_workspace(n, c) for n, c in ((5, 8), (5, 240), (1, 16), (2 ** 24 + 1, 16))] == [-2, -2, -1, -1]
    assert lib.cg_bn_relu_train_forward(None, 5, 16, None, None, 1e-5, None, None, None, None, None, None, None, None) == -1
    assert lib.cg_bn_relu_train_forward(None, 5, 8, None, None, 1e-5, None, None, None, None, None, None, None, None) == -2
    assert lib.cg_bn_relu_train_backward(None, None, 1, 16, None, None, None, None, None, None, None, None, None) == -1
    assert lib.cg_bn_relu_train_backward(None, None, 5, 240, None, None, None, None, None, None, None, None, None) == -2
    for sigs in (_lib.signatures(), _lib.cluster_signatures(), _lib.sparse_signatures(), _lib.pointgroup_signatures(), _lib.scene_signatures(),
                 _lib.neighbors_signatures(), _lib.kdtree_signatures(), _lib.sparse_grad_signatures()):
        assert not set(BN_SYMBOLS) & set(sigs)


def test_lib_raises_when_the_library_lacks_a_bn_symbol(monkeypatch):
    real = _lib.bn_signatures()
    monkeypatch.setattr(_lib, '_lib', None)
    monkeypatch.setattr(_lib, 'bn_signatures', lambda: {**real, 'cg_bn_not_built': (ctypes.c_int, ())})
    with pytest.raises(_lib.CatgraspAmdError, match='cg_bn_not_built'):
        _lib.lib()


def test_build_tracks_the_bn_header_and_compiles_the_kernels():
    from catgrasp_amd import build
    assert 'catgrasp_amd_bn.h' in inspect.getsource(build.build)
    src = [s for s in build.sources() if s.endswith('batchnorm_train.hip')]
    assert len(src) == 1
    with open(src[0]) as f:
        text = re.sub(r'//.*', '', f.read())
    assert 'catgrasp_amd_bn.h' in text and 'fmaf(' in text and 'atomic' not in text and 'asm' not in text
    assert '-ffp-contract=off' in build.FLAGS


def test_the_wrapper_refuses_what_is_not_built_before_any_device_work():
    bn = nn.BatchNorm1d(16).train()
    with pytest.raises(NotImplementedError, match='HIP device'):
        batchnorm.bn_relu_train(torch.zeros(4, 16), bn)                                      # host tensors: no CPU fallback
    with pytest.raises(NotImplementedError):
        batchnorm.bn_relu_train(torch.zeros(4, 16), nn.BatchNorm1d(16, momentum=None).train())
    with pytest.raises(NotImplementedError):
        batchnorm.bn_relu_train(torch.zeros(4, 16), nn.BatchNorm1d(16, affine=False).train())
    with pytest.raises(NotImplementedError):
        batchnorm.bn_relu_train(torch.zeros(4, 16), nn.BatchNorm1d(16, track_running_stats=False).train())
    with pytest.raises(ValueError, match='training mode'):
        batchnorm.bn_relu_train(torch.zeros(4, 16), bn.eval())
    with pytest.raises(ValueError):
        batchnorm.bn_relu_train(torch.zeros(4, 32), bn.train())
