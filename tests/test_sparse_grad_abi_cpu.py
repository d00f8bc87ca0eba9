"""CPU tests (no GPU) of the boundary of the sparse convolution layers' gradients: include/catgrasp_amd_sparse_grad.h is plain C99, alone
and next to the other seven headers in either order, and links from C; every argument error comes back without a GPU; the workspace
size is a function of the shapes; the ctypes binding takes its types from that header and lib() requires its symbols; the build tracks
it; the Python layers refuse to run without a HIP device, carry the base layers' state_dict layout, and leave the inference module's
refusal under enabled gradients where it was."""
import ctypes
import inspect
import os
import re
import shutil
import subprocess

import pytest
import torch

import catgrasp_amd.spconv as base
import catgrasp_amd.spconv_autograd as spconv
from catgrasp_amd import _lib

INCLUDE = os.path.dirname(_lib.SPARSE_GRAD_HEADER_PATH)
GRAD_SYMBOLS = ['cg_sparse_conv_dgrad', 'cg_sparse_conv_wgrad', 'cg_sparse_wgrad_workspace']
HEADERS = ['catgrasp_amd.h', 'catgrasp_amd_cluster.h', 'catgrasp_amd_sparse.h', 'catgrasp_amd_pointgroup.h', 'catgrasp_amd_scene.h',
           'catgrasp_amd_neighbors.h', 'catgrasp_amd_kdtree.h', 'catgrasp_amd_sparse_grad.h']
GCC = ['gcc', '-std=c99', '-Wall', '-Wextra', '-Werror', '-pedantic', '-I', INCLUDE]


def test_grad_header_is_strict_c99_alone_and_with_the_others_and_links_from_c(tmp_path):
    if shutil.which('gcc') is None:
        pytest.fail('gcc is needed to check the header')
    assert sorted(_lib.sparse_grad_signatures()) == GRAD_SYMBOLS
    wgrad = 'cg_sparse_conv_wgrad({x}, {n_in}, {nbr}, {n_out}, {K}, {dy}, {cin}, {cout}, {ws}, {dw}, {db}, (void*)0)'
    dgrad = 'cg_sparse_conv_dgrad({dy}, {n_out}, {nbr}, {n_in}, {K}, {w}, {cin}, {cout}, {dx}, (void*)0)'
    good = dict(x='f', n_in='4L', nbr='i', n_out='4L', K='27', dy='f', cin='16', cout='16', ws='f', dw='f', db='f', w='f', dx='f')
    # the host arrays stand in for device memory: nothing may be launched, so nothing reads them
    cases = [(wgrad, b, 'CG_ERR_ARG') for b in (dict(x='(float*)0'), dict(nbr='(int*)0'), dict(dy='(float*)0'), dict(dw='(float*)0', db='(float*)0'),
                                                dict(ws='(float*)0'),                      # no workspace with n_out > 0
                                                dict(n_in='-1L'), dict(n_out='-1L'), dict(K='9'), dict(K='0'), dict(cin='0'), dict(cout='-16'))]
    cases += [(dgrad, b, 'CG_ERR_ARG') for b in (dict(dy='(float*)0'), dict(nbr='(int*)0'), dict(w='(float*)0'), dict(dx='(float*)0'), dict(n_in='-1L'),
                                                dict(n_out='-1L'), dict(K='9'), dict(cin='0'))]
    for call in (wgrad, dgrad):
        cases += [(call, b, 'CG_ERR_UNSUPPORTED') for b in (dict(cin='17'), dict(cout='128'), dict(cin='17', cout='128'), dict(cin='3'), dict(cout='6'),
                                                           dict(cin='240'), dict(cin='8'))]
        cases += [(call, dict(K='9', cin='17'), 'CG_ERR_ARG')]                              # the count is judged before the channel set
    # no rows: nothing to launch.  (cg_sparse_conv_wgrad with n_out = 0 zeroes dw and db with a device memset; it is not called here
    # with host memory standing in: tests/test_sparse_grad_gpu.py checks its zeros and its CG_OK on the device.)
    cases += [(dgrad, dict(n_in='0L', dx='(float*)0', nbr='(int*)0'), 'CG_OK'), (dgrad, dict(n_in='0L', n_out='0L', dy='(float*)0'), 'CG_OK')]
    body = ''.join(f'  bad += {call.format(**{**good, **b})} != {want};   /* {b} */\n' for call, b, want in cases)
    rows = spconv.grad_rows()
    sizes = [(0, 0), (1, 1), (rows, 1), (rows + 1, 2)]
    for n, chunks in sizes:
        body += f'  bad += cg_sparse_wgrad_workspace({n}L, 27, 16, 32) != {chunks}L * (27L * 16 * 32 + 32);\n'
    body += ('  bad += cg_sparse_wgrad_workspace(2L * CG_SPARSE_GRAD_ROWS + 1, 8, 6, 3) != 3L * (8 * 6 * 3 + 3);\n'
             '  bad += cg_sparse_wgrad_workspace(5L, 9, 16, 16) != CG_ERR_ARG;\n  bad += cg_sparse_wgrad_workspace(-1L, 27, 16, 16) != CG_ERR_ARG;\n'
             '  bad += cg_sparse_wgrad_workspace(5L, 27, 17, 128) != CG_ERR_UNSUPPORTED;\n')
    for n, order in enumerate((HEADERS, HEADERS[::-1])):
        src = (''.join(f'#include "{h}"\n' for h in order) + '#include "catgrasp_amd_sparse_grad.h"\n#include <stdio.h>\n'
               'typedef void (*fn_t)(void);\nint main(void) {\n  fn_t table[] = {\n' + ''.join(f'    (fn_t)&{s},\n' for s in GRAD_SYMBOLS)
               + '  };\n  float f[4]; int i[4];\n  int bad = 0;\n  f[0] = 0.f; i[0] = 0;\n' + body
               + '  printf("%d %d\\n", (int)(sizeof table / sizeof table[0]), CG_SPARSE_GRAD_ROWS);\n  return bad;\n}\n')
        (tmp_path / f'main{n}.c').write_text(src)
        libdir = os.path.dirname(_lib.LIB_PATH)
        subprocess.check_call(GCC + [f'main{n}.c', '-L', libdir, '-lcatgrasp_amd', f'-Wl,-rpath,{libdir}', '-Wl,--allow-shlib-undefined', '-o', f'main{n}'],
                              cwd=tmp_path)
        out = subprocess.run([str(tmp_path / f'main{n}')], capture_output=True, text=True)
        assert out.returncode == 0, (out.returncode, out.stdout, out.stderr)
        assert out.stdout.split() == ['3', str(rows)] and rows % 64 == 0
    (tmp_path / 'alone.c').write_text('#include "catgrasp_amd_sparse_grad.h"\nint main(void) { return CG_OK; }\n')
    subprocess.check_call(GCC + ['-fsyntax-only', 'alone.c'], cwd=tmp_path)


def test_binding_takes_the_grad_types_from_the_header_and_leaves_the_other_headers_alone():
    lib = _lib.lib()
    vp, ci, cl = ctypes.c_void_p, ctypes.c_int, ctypes.c_long
    with open(_lib.SPARSE_GRAD_HEADER_PATH) as f:
        text = re.sub(r'/\*.*?\*/', '', f.read(), flags=re.S)
    for name in GRAD_SYMBOLS:
        m = re.search(r'\b(int|long)\s+' + name + r'\s*\(([^)]*)\)\s*;', text)
        params = [' '.join(q.split()) for q in m.group(2).split(',')]
        fn = getattr(lib, name)
        assert fn.restype is {'int': ci, 'long': cl}[m.group(1)] and len(fn.argtypes) == len(params), name
        for at, q in zip(fn.argtypes, params):
            assert at is (vp if '*' in q else {'int': ci, 'long': cl}[q.rsplit(' ', 1)[0]]), (name, q)
    assert tuple(lib.cg_sparse_wgrad_workspace.argtypes) == (cl, ci, ci, ci) and lib.cg_sparse_wgrad_workspace.restype is cl
    assert tuple(lib.cg_sparse_conv_wgrad.argtypes) == (vp, cl, vp, cl, ci, vp, ci, ci, vp, vp, vp, vp)
    assert tuple(lib.cg_sparse_conv_dgrad.argtypes) == (vp, cl, vp, cl, ci, vp, ci, ci, vp, vp)
    with pytest.raises(ctypes.ArgumentError):
        lib.cg_sparse_conv_wgrad(None, 1, None, 1, 27.0, None, 16, 16, None, None, None, None)        # a float for K never reaches C
    assert lib.cg_sparse_conv_wgrad(None, 1, None, 1, 27, None, 16, 16, None, None, None, None) == -1
    assert lib.cg_sparse_conv_wgrad(None, 1, None, 1, 27, None, 17, 128, None, None, None, None) == -2
    assert lib.cg_sparse_conv_dgrad(None, 1, None, 1, 27, None, 16, 16, None, None) == -1
    assert lib.cg_sparse_conv_dgrad(None, 1, None, 1, 9, None, 16, 16, None, None) == -1
    assert lib.cg_sparse_conv_dgrad(None, 1, None, 0, 27, None, 224, 112, None, None) == 0           # no rows to write
    rows = spconv.grad_rows()
    assert [lib.cg_sparse_wgrad_workspace(n, 27, 224, 112) for n in (0, 1, rows, rows + 1)] == [c * (27 * 224 * 112 + 112) for c in (0, 1, 1, 2)]
    assert lib.cg_sparse_wgrad_workspace(2 ** 26, 27, 224, 112) == 2 ** 16 * (27 * 224 * 112 + 112)      # a long comes back intact
    assert lib.cg_sparse_wgrad_workspace(2 ** 26 + 1, 27, 224, 112) == -1
    # the other headers' views are unchanged
    assert len(_lib.declared_symbols()) == 71
    assert sorted(_lib.sparse_signatures()) == ['cg_sparse_conv', 'cg_sparse_keys', 'cg_sparse_rules_down', 'cg_sparse_rules_inverse', 'cg_sparse_rules_subm']
    for sigs in (_lib.signatures(), _lib.cluster_signatures(), _lib.sparse_signatures(), _lib.pointgroup_signatures(), _lib.scene_signatures(),
                 _lib.neighbors_signatures(), _lib.kdtree_signatures()):
        assert not set(GRAD_SYMBOLS) & set(sigs)


def test_lib_raises_when_the_library_lacks_a_grad_symbol(monkeypatch):
    real = _lib.sparse_grad_signatures()
    monkeypatch.setattr(_lib, '_lib', None)
    monkeypatch.setattr(_lib, 'sparse_grad_signatures', lambda: {**real, 'cg_sparse_grad_not_built': (ctypes.c_int, ())})
    with pytest.raises(_lib.CatgraspAmdError, match='cg_sparse_grad_not_built'):
        _lib.lib()


def test_build_tracks_the_grad_header_and_compiles_the_kernels():
    from catgrasp_amd import build
    assert 'catgrasp_amd_sparse_grad.h' in inspect.getsource(build.build)
    src = [s for s in build.sources() if s.endswith('sparse_conv_grad.hip')]
    assert len(src) == 1
    with open(src[0]) as f:
        text = re.sub(r'//.*', '', f.read())
    assert 'catgrasp_amd_sparse_grad.h' in text and 'mfma32(' in text and 'atomic' not in text and 'asm' not in text
    assert 'eight' in _lib.__doc__


def _tensor(c):
    return spconv.SparseConvTensor(torch.zeros(3, c), torch.tensor([[0, 0, 0, 0], [0, 1, 1, 1], [1, 2, 2, 2]], dtype=torch.int32), [9, 12, 17], 2)


def test_the_layers_raise_without_a_hip_device_with_and_without_gradients(monkeypatch):
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)          # on a GPU host too: the refusal, not a CPU fallback
    layers = [spconv.SubMConv3d(16, 16, 3, padding=1), spconv.SubMConv3d(16, 16, 1), spconv.SparseConv3d(16, 32, 2, stride=2, indice_key='k'),
              spconv.SparseConv3d(16, 32, 2, stride=2), spconv.SparseInverseConv3d(16, 32, 2, indice_key='k')]
    for layer in layers:
        assert layer.weight.requires_grad
        with pytest.raises(_lib.CatgraspAmdError, match='HIP device'):
            layer(_tensor(16))                                              # gradients enabled: the differentiable path
        with torch.no_grad(), pytest.raises(_lib.CatgraspAmdError, match='HIP device'):
            layer(_tensor(16))                                              # and the base class's
    with pytest.raises(TypeError):
        layers[0](torch.zeros(3, 16))


def test_state_dicts_are_the_base_layers_and_load_strictly_both_ways():
    assert spconv.SparseConvTensor is base.SparseConvTensor and spconv.SparseSequential is base.SparseSequential
    assert spconv.SparseModule is base.SparseModule and spconv.RuleBook is base.RuleBook
    assert spconv.subm_rules is base.subm_rules and spconv.down_rules is base.down_rules and spconv.inverse_rules is base.inverse_rules
    cases = [('SubMConv3d', (32, 16, 3), dict(padding=1, indice_key='subm1')), ('SubMConv3d', (6, 16, 1), dict(bias=False)),
             ('SparseConv3d', (16, 32, 2), dict(stride=2, indice_key='spconv1')), ('SparseInverseConv3d', (32, 16, 2), dict(indice_key='spconv1'))]
    for name, args, kw in cases:
        torch.manual_seed(3)
        new = getattr(spconv, name)(*args, **kw)
        torch.manual_seed(3)
        old = getattr(base, name)(*args, **kw)
        assert isinstance(new, getattr(base, name)) and isinstance(new, spconv.SparseModule)
        a, b = new.state_dict(), old.state_dict()
        assert list(a) == list(b) and all(a[k].shape == b[k].shape and torch.equal(a[k], b[k]) for k in a)      # same keys, shapes, initialisation
        with torch.no_grad():
            new.weight.add_(1.0)
        old.load_state_dict(new.state_dict(), strict=True)
        assert torch.equal(old.weight, new.weight)
        new.load_state_dict(old.state_dict(), strict=True)
        assert [n for n, _ in new.named_parameters()] == [n for n, _ in old.named_parameters()]
    for make in (lambda: spconv.SubMConv3d(16, 16, 5, padding=2), lambda: spconv.SparseConv3d(16, 32, 3, stride=2)):
        with pytest.raises(NotImplementedError):
            make()
    with pytest.raises(ValueError):
        spconv.SubMConv3d(8, 16, 3, padding=1)


class _DeviceRows:
    """Stands where device features would, up to the refusal: it comes before any device work."""
    is_cuda, requires_grad, dtype, shape = True, False, torch.float32, (3, 16)

    def __getattr__(self, name):
        raise AssertionError(f'device work ({name}) before the refusal')


def test_the_inference_module_still_refuses_enabled_gradients(monkeypatch):
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: True)
    x = _tensor(16)
    x.features = x.indices = _DeviceRows()
    for layer in (base.SubMConv3d(16, 16, 3, padding=1), base.SparseConv3d(16, 32, 2, stride=2), base.SparseInverseConv3d(16, 32, 2, indice_key='k')):
        with pytest.raises(NotImplementedError, match='inference only'):
            layer(x)
    # and the differentiable layers refuse what they do not differentiate, before any device work
    with pytest.raises(NotImplementedError, match='features_b'):
        spconv.SubMConv3d(32, 16, 3, padding=1)(x, features_b=torch.zeros(3, 16))
