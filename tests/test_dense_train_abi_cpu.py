"""CPU tests (no GPU) of the boundary of the dense layers' gradients: catgrasp_amd/include/catgrasp_amd_dense.h is plain C99, alone and
after the headers of include/ in either order, and links from C; every argument error and every limit comes back without a GPU; the
workspace sizes are the stated functions of the shapes; the ctypes binding takes its types from that header and lib() requires its
symbols; the build tracks it; the kernels stay out of scratch; the Python wrappers refuse what they do not build before any device
work."""
import ctypes
import inspect
import os
import re
import shutil
import subprocess

import pytest
import torch
from torch import nn

from catgrasp_amd import _lib, batchnorm, dense_autograd as D, pointnet2_train

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.dirname(_lib.HEADER_PATH)
PKG_INCLUDE = os.path.dirname(_lib.DENSE_HEADER_PATH)
SYMBOLS = ['cg_bn_relu_train_backward_wide', 'cg_bn_relu_train_forward_wide', 'cg_bn_wide_workspace', 'cg_dense_dgrad', 'cg_dense_group_sums',
           'cg_dense_group_sums_workspace', 'cg_dense_wgrad', 'cg_dense_wgrad_workspace']
HEADERS = ['catgrasp_amd.h', 'catgrasp_amd_cluster.h', 'catgrasp_amd_sparse.h', 'catgrasp_amd_pointgroup.h', 'catgrasp_amd_scene.h',
           'catgrasp_amd_neighbors.h', 'catgrasp_amd_kdtree.h', 'catgrasp_amd_sparse_grad.h', 'catgrasp_amd_bn.h', 'catgrasp_amd_screen.h',
           'catgrasp_amd_loss.h']
GCC = ['gcc', '-std=c99', '-Wall', '-Wextra', '-Werror', '-pedantic', '-I', INCLUDE, '-I', PKG_INCLUDE]
R = 1024          # CG_DENSE_GRAD_ROWS, printed by the C program below


def test_dense_header_is_strict_c99_alone_and_after_the_others_and_links_from_c(tmp_path):
    if shutil.which('gcc') is None:
        pytest.fail('gcc is needed to check the header')
    assert sorted(_lib.dense_signatures()) == SYMBOLS
    assert os.path.samefile(os.path.dirname(PKG_INCLUDE), os.path.dirname(_lib.__file__)) and not os.path.samefile(PKG_INCLUDE, INCLUDE)
    wg = 'cg_dense_wgrad({x}, {dy}, {n}, {cin}, {cout}, {ws}, {dw}, {db}, (void*)0)'
    dg = 'cg_dense_dgrad({dy}, {n}, {cout}, {w}, {cin}, {dx}, (void*)0)'
    gs = 'cg_dense_group_sums({dy}, {g}, {rpg}, {c}, {ws}, {s}, (void*)0)'
    fwd = 'cg_bn_relu_train_forward_wide({x}, {n}, {c}, f, f, 1e-5f, {ws}, f, f, f, f, f, f, (void*)0)'
    bwd = 'cg_bn_relu_train_backward_wide({x}, {dy}, {n}, {c}, f, f, f, f, {ws}, f, f, f, (void*)0)'
    good = dict(x='f', dy='f', n='4L', cin='8', cout='4', ws='f', dw='f', db='f', w='f', dx='f', g='2L', rpg='3L', c='16', s='f')
    null, odd = '(float*)0', '(f + 1)'          # the host array stands in for device memory: nothing may be launched, so nothing reads it
    cases = [(wg, b, 'CG_ERR_ARG') for b in (dict(dy=null), dict(ws=null), dict(x=null), dict(dw=null, db=null), dict(dy=odd), dict(x=odd),
                                             dict(n='0L'), dict(n='-1L'), dict(n='16777217L'), dict(cin='0'), dict(cout='-4'))]
    cases += [(wg, b, 'CG_ERR_UNSUPPORTED') for b in (dict(cin='4'), dict(cin='12'), dict(cin='1032'), dict(cout='6'), dict(cout='1028'))]
    cases += [(wg, dict(n='0L', cin='4'), 'CG_ERR_ARG')]                                       # the count is judged before the widths
    cases += [(dg, b, 'CG_ERR_ARG') for b in (dict(dy=null), dict(w=null), dict(dx=null), dict(dy=odd), dict(n='0L'), dict(n='16777217L'),
                                             dict(cin='0'), dict(cout='0'))]
    cases += [(dg, b, 'CG_ERR_UNSUPPORTED') for b in (dict(cin='6'), dict(cin='1028'), dict(cout='6'), dict(cout='1028'))]
    cases += [(gs, b, 'CG_ERR_ARG') for b in (dict(dy=null), dict(s=null), dict(ws=null, rpg='1025L'), dict(g='0L'), dict(rpg='0L'),
                                             dict(g='4097L', rpg='4096L'), dict(g='16777217L', rpg='1L'), dict(c='0'))]
    cases += [(gs, b, 'CG_ERR_UNSUPPORTED') for b in (dict(c='6'), dict(c='1028'))]
    for call in (fwd, bwd):
        cases += [(call, b, 'CG_ERR_ARG') for b in (dict(x=null), dict(ws=null), dict(n='1L'), dict(n='16777217L'), dict(c='0'))]
        cases += [(call, dict(c=c), 'CG_ERR_UNSUPPORTED') for c in ('8', '17', '1040', '2048')]
    body = ''.join(f'  bad += {call.format(**{**good, **b})} != {want};   /* {b} */\n' for call, b, want in cases)
    for n, cin, cout, want in ((1, 8, 4, 36), (R, 8, 4, 36), (R + 1, 8, 4, 72), (2 * R + 1, 128, 300, 3 * (128 * 300 + 300)),
                               (16777216, 1024, 1024, (16777216 // R) * (1024 * 1024 + 1024))):
        body += f'  bad += cg_dense_wgrad_workspace({n}L, {cin}, {cout}) != {want}L;\n'
    for g, rpg, c, want in ((1, 1, 4, 4), (3, 1024, 12, 36), (3, 1025, 12, 72), (34, 8192, 512, 34 * 512 * 8)):
        body += f'  bad += cg_dense_group_sums_workspace({g}L, {rpg}L, {c}) != {want}L;\n'
    for n, c, want in ((2, 240, 480), (1025, 512, 2048), (16777216, 1024, 2 * 1024 * 16384)):
        body += f'  bad += cg_bn_wide_workspace({n}L, {c}) != {want}L;\n'
    body += ('  bad += cg_dense_wgrad_workspace(5L, 12, 4) != CG_ERR_UNSUPPORTED;\n  bad += cg_dense_wgrad_workspace(0L, 8, 4) != CG_ERR_ARG;\n'
             '  bad += cg_dense_group_sums_workspace(1L, 1L, 6) != CG_ERR_UNSUPPORTED;\n  bad += cg_dense_group_sums_workspace(0L, 1L, 4) != CG_ERR_ARG;\n'
             '  bad += cg_bn_wide_workspace(5L, 1040) != CG_ERR_UNSUPPORTED;\n  bad += cg_bn_wide_workspace(1L, 16) != CG_ERR_ARG;\n'
             '  bad += cg_bn_workspace(5L, 240) != CG_ERR_UNSUPPORTED;\n')                     # the narrow entry points keep their limit
    for k, order in enumerate((HEADERS, HEADERS[::-1])):
        src = (''.join(f'#include "{h}"\n' for h in order) + '#include "catgrasp_amd_dense.h"\n#include <stdio.h>\n'
               'typedef void (*fn_t)(void);\nint main(void) {\n  fn_t table[] = {\n' + ''.join(f'    (fn_t)&{s},\n' for s in SYMBOLS)
               + '  };\n  float f[8];\n  int bad = 0;\n  f[0] = 0.f;\n' + body
               + '  printf("%d %d %d\\n", (int)(sizeof table / sizeof table[0]), CG_DENSE_GRAD_ROWS, CG_DENSE_MAX_C);\n  return bad;\n}\n')
        (tmp_path / f'main{k}.c').write_text(src)
        libdir = os.path.dirname(_lib.LIB_PATH)
        subprocess.check_call(GCC + [f'main{k}.c', '-L', libdir, '-lcatgrasp_amd', f'-Wl,-rpath,{libdir}', '-Wl,--allow-shlib-undefined', '-o', f'main{k}'],
                              cwd=tmp_path)
        out = subprocess.run([str(tmp_path / f'main{k}')], capture_output=True, text=True)
        assert out.returncode == 0, (out.returncode, out.stdout, out.stderr)
        assert out.stdout.split() == [str(len(SYMBOLS)), str(R), '1024']
    (tmp_path / 'alone.c').write_text('#include "catgrasp_amd_dense.h"\nint main(void) { return CG_OK; }\n')
    subprocess.check_call(GCC + ['-fsyntax-only', 'alone.c'], cwd=tmp_path)


def test_binding_takes_the_dense_types_from_the_header():
    lib = _lib.lib()
    vp, ci, cl, cf = ctypes.c_void_p, ctypes.c_int, ctypes.c_long, ctypes.c_float
    scalar = {'int': ci, 'long': cl, 'float': cf}
    with open(_lib.DENSE_HEADER_PATH) as f:
        text = re.sub(r'/\*.*?\*/', '', f.read(), flags=re.S)
    for name in SYMBOLS:
        m = re.search(r'\b(int|long)\s+' + name + r'\s*\(([^)]*)\)\s*;', text)
        params = [' '.join(q.split()) for q in m.group(2).split(',')]
        fn = getattr(lib, name)
        assert fn.restype is scalar[m.group(1)] and len(fn.argtypes) == len(params), name
        for at, q in zip(fn.argtypes, params):
            assert at is (vp if '*' in q else scalar[q.rsplit(' ', 1)[0]]), (name, q)
    assert tuple(lib.cg_dense_wgrad.argtypes) == (vp, vp, cl, ci, ci, vp, vp, vp, vp)
    assert tuple(lib.cg_dense_dgrad.argtypes) == (vp, cl, ci, vp, ci, vp, vp)
    assert tuple(lib.cg_dense_group_sums.argtypes) == (vp, cl, cl, ci, vp, vp, vp)
    assert tuple(lib.cg_bn_relu_train_forward_wide.argtypes) == tuple(lib.cg_bn_relu_train_forward.argtypes)
    assert tuple(lib.cg_bn_relu_train_backward_wide.argtypes) == tuple(lib.cg_bn_relu_train_backward.argtypes)
    with pytest.raises(ctypes.ArgumentError):
        lib.cg_dense_wgrad_workspace(5, 8.0, 4)                                               # a float for cin never reaches C
    assert [lib.cg_dense_wgrad_workspace(n, 64, 36) for n in (1, R, R + 1, 2 * R + 1)] == [k * (64 * 36 + 36) for k in (1, 1, 2, 3)]
    assert D.grad_rows() == R
    assert lib.cg_dense_wgrad(None, None, 5, 8, 4, None, None, None, None) == -1
    assert lib.cg_dense_wgrad(None, None, 5, 12, 4, None, None, None, None) == -2
    assert lib.cg_dense_dgrad(None, 5, 300, None, 128, None, None) == -1
    assert lib.cg_dense_dgrad(None, 5, 302, None, 128, None, None) == -2
    assert lib.cg_dense_group_sums(None, 2, 3, 12, None, None, None) == -1
    assert [lib.cg_bn_wide_workspace(n, c) for n, c in ((5, 512), (5, 1024), (5, 1040), (5, 8), (1, 16))] == [1024, 2048, -2, -2, -1]
    assert lib.cg_bn_relu_train_forward_wide(None, 5, 512, None, None, 1e-5, None, None, None, None, None, None, None, None) == -1
    assert lib.cg_bn_relu_train_backward_wide(None, None, 5, 1040, None, None, None, None, None, None, None, None, None) == -2
    for sigs in (_lib.signatures(), _lib.bn_signatures(), _lib.sparse_grad_signatures(), _lib.loss_signatures()):
        assert not set(SYMBOLS) & set(sigs)


def test_lib_raises_when_the_library_lacks_a_dense_symbol(monkeypatch):
    real = _lib.dense_signatures()
    monkeypatch.setattr(_lib, '_lib', None)
    monkeypatch.setattr(_lib, 'dense_signatures', lambda: {**real, 'cg_dense_not_built': (ctypes.c_int, ())})
    with pytest.raises(_lib.CatgraspAmdError, match='cg_dense_not_built'):
        _lib.lib()


def test_build_tracks_the_dense_header_and_compiles_the_kernels():
    from catgrasp_amd import build
    assert 'catgrasp_amd_dense.h' in inspect.getsource(build.build)
    src = [s for s in build.sources() if s.endswith('dense_train.hip')]
    assert len(src) == 1
    with open(src[0]) as f:
        text = f.read()
    assert 'catgrasp_amd_dense.h' in text and 'fmaf(' in text and 'atomic' not in text and 'asm' not in text
    assert '-ffp-contract=off' in build.FLAGS
    with open(os.path.join(ROOT, '.gitignore')) as f:
        assert not any(line.strip().rstrip('/') in ('include', 'catgrasp_amd/include', '*.h') for line in f)


def test_the_new_kernels_stay_out_of_scratch():
    """Code-object metadata of the built gfx950 image (scripts/kernel_resources.py; no GPU needed): no private segment, no spilled
    registers in any kernel of dense_train.hip and batchnorm_train.hip."""
    import importlib.util
    spec = importlib.util.spec_from_file_location('kernel_resources', os.path.join(ROOT, 'scripts', 'kernel_resources.py'))
    kr = importlib.util.module_from_spec(spec); spec.loader.exec_module(kr)
    if not all(os.path.exists(os.path.join(kr.LLVM, t)) for t in ('llvm-objcopy', 'clang-offload-bundler', 'llvm-readelf')) or shutil.which('c++filt') is None:
        pytest.skip('ROCm llvm binutils / c++filt not found')
    seen = []
    for obj in ('dense_train.o', 'batchnorm_train.o'):
        path = os.path.join(ROOT, 'catgrasp_amd', 'csrc', obj)
        if not os.path.exists(path):
            pytest.skip(f'{obj} not built')
        for r in kr.resources(path):
            seen.append(r['kernel'].replace('void ', ''))
            assert r['private_segment_fixed_size'] == 0 and r['vgpr_spill_count'] == 0 and r['sgpr_spill_count'] == 0, r
    for k in ('dense_wgrad_kernel<1>', 'dense_wgrad_kernel<2>', 'dense_wgrad_kernel<4>', 'dense_wgrad_reduce_kernel', 'dense_dgrad_kernel',
              'dense_group_sum_kernel', 'dense_group_total_kernel', 'bn_apply_kernel'):
        assert any(s.startswith(k) for s in seen), (k, seen)


def test_the_wrappers_refuse_what_is_not_built_before_any_device_work():
    x, w = torch.zeros(4, 8), torch.zeros(4, 8)
    with pytest.raises(NotImplementedError, match='HIP device'):
        D.linear(x, w)                                                                        # host tensors: no CPU fallback
    with pytest.raises(NotImplementedError, match='HIP device'):
        D.linear_group_bias(x, w, None, torch.zeros(2, 4), 2)
    for fn, args in ((D.dense_wgrad, (x, torch.zeros(4, 4))), (D.dense_dgrad, (torch.zeros(4, 4), w)), (D.group_sums, (x, 2)),
                     (D.dense_forward, (x, w))):
        with pytest.raises(NotImplementedError, match='HIP device'):
            fn(*args)
    with pytest.raises(NotImplementedError, match='float32'):
        D.linear(x.double(), w.double())
    convs = [nn.Conv1d(a, b, 1) for a, b in ((48, 32), (32, 16), (16, 16), (16, 12))]
    bns = [nn.BatchNorm1d(c) for c in (32, 16, 16)]
    with pytest.raises(NotImplementedError, match='HIP device'):
        D.seg_head_train(torch.zeros(2, 32), torch.zeros(2, 5, 16), convs, bns)
    with pytest.raises(ValueError):
        D.seg_head_train(torch.zeros(2, 32), torch.zeros(2, 5, 16), convs[:3], bns)
    bn = nn.BatchNorm1d(512).train()
    with pytest.raises(NotImplementedError, match='HIP device'):
        batchnorm.bn_relu_train(torch.zeros(4, 512), bn)
    model = pointnet2_train.PointNetSeg(6, 12).train()
    with pytest.raises(NotImplementedError, match='HIP device'):
        model(torch.zeros(2, 8, 6))
    with pytest.raises(NotImplementedError, match='float32'):
        model(torch.zeros(2, 8, 6, dtype=torch.float64))
    assert pointnet2_train.USE_TORCH_OPS is False


def test_raw_wrappers_refuse_non_contiguous_inputs_on_the_host(monkeypatch):
    """The raw wrappers judge dtype, strides and device, in that order, before lib() is touched."""
    class FakeLib:
        def __getattr__(self, name):
            raise AssertionError(f'{name} was reached')
    monkeypatch.setattr(_lib, 'lib', lambda: FakeLib())
    t = torch.zeros(8, 4).t()
    assert not t.is_contiguous()
    with pytest.raises(ValueError, match='contiguous'):
        D.dense_wgrad(t, torch.zeros(4, 4))
    with pytest.raises(ValueError, match='contiguous'):
        D.dense_dgrad(torch.zeros(4, 8)[:, ::2], torch.zeros(4, 8))
    with pytest.raises(ValueError, match='contiguous'):
        D.group_sums(t, 2)
    with pytest.raises(ValueError, match='contiguous'):
        D.dense_forward(t, torch.zeros(4, 8))
    with pytest.raises(NotImplementedError, match='float32'):
        D.dense_wgrad(torch.zeros(4, 8, dtype=torch.float64), torch.zeros(4, 4))
    with pytest.raises(NotImplementedError, match='HIP device'):
        D.dense_wgrad(torch.zeros(4, 8), torch.zeros(4, 4))


def test_the_trainable_model_has_the_reference_modules_and_initial_tensors():
    from catgrasp_amd import pointnet2
    torch.manual_seed(3)
    base = pointnet2.PointNetSeg(6, 300)
    torch.manual_seed(3)
    ours = pointnet2_train.PointNetSeg(6, 300)
    a, b = base.state_dict(), ours.state_dict()
    assert list(a) == list(b)
    for k in a:
        assert a[k].shape == b[k].shape and torch.equal(a[k], b[k]), k
    assert [n for n, _ in base.named_modules()] == [n for n, _ in ours.named_modules()]
    base.load_state_dict(ours.state_dict(), strict=True)
