"""CPU tests (no GPU) of the boundary of the pooled layer's closed-form training: catgrasp_amd/include/catgrasp_amd_pool.h is plain C99,
alone and after the twelve other headers in either order, and links from C; its symbols are its own; every argument error and every
limit comes back without a GPU; the workspace size is the stated function of the shapes; the ctypes binding takes its types from that
header and lib() requires its symbols; the build tracks it; the kernels stay out of scratch; the Python wrappers refuse host tensors
before any device work."""
import ctypes
import inspect
import os
import shutil
import subprocess

import pytest
import torch
from torch import nn

from catgrasp_amd import _lib, pointnet2_train, pool_autograd as PA

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.dirname(_lib.HEADER_PATH)
PKG_INCLUDE = os.path.dirname(_lib.POOL_HEADER_PATH)
SYMBOLS = ['cg_pool_dgrad_scatter', 'cg_pool_extrema', 'cg_pool_extrema_workspace', 'cg_pool_stats', 'cg_pool_var', 'cg_pool_var_workspace',
           'cg_pool_wgrad_gather']
HEADERS = ['catgrasp_amd.h', 'catgrasp_amd_cluster.h', 'catgrasp_amd_sparse.h', 'catgrasp_amd_pointgroup.h', 'catgrasp_amd_scene.h',
           'catgrasp_amd_neighbors.h', 'catgrasp_amd_kdtree.h', 'catgrasp_amd_sparse_grad.h', 'catgrasp_amd_bn.h', 'catgrasp_amd_screen.h',
           'catgrasp_amd_loss.h', 'catgrasp_amd_dense.h']
OTHERS = ('signatures', 'cluster_signatures', 'sparse_signatures', 'pointgroup_signatures', 'scene_signatures', 'neighbors_signatures',
          'kdtree_signatures', 'sparse_grad_signatures', 'bn_signatures', 'screen_signatures', 'loss_signatures', 'dense_signatures')
GCC = ['gcc', '-std=c99', '-Wall', '-Wextra', '-Werror', '-pedantic', '-I', INCLUDE, '-I', PKG_INCLUDE]


def test_pool_header_is_strict_c99_alone_and_after_the_others_and_refuses_from_c(tmp_path):
    if shutil.which('gcc') is None:
        pytest.fail('gcc is needed to check the header')
    assert sorted(_lib.pool_signatures()) == SYMBOLS and len(HEADERS) == len(OTHERS) == 12
    assert os.path.samefile(PKG_INCLUDE, os.path.dirname(_lib.DENSE_HEADER_PATH))
    ex = 'cg_pool_extrema({x}, {b}, {n}, {cin}, {wp}, f, {c}, f, {ws}, {z}, {i}, (void*)0)'
    st = 'cg_pool_stats({w}, f, {xbar}, {s}, {vin}, f, f, 1e-5f, {b}, {n}, {cin}, {c}, {z}, 1, {mean}, f, f, f, f, {out}, (void*)0)'
    va = 'cg_pool_var({x}, {b}, {n}, {cin}, {wp}, f, {c}, {mean}, {ws}, {var}, (void*)0)'
    ga = 'cg_pool_wgrad_gather({x}, {b}, {n}, {cin}, {coef}, {i}, {c}, {t}, (void*)0)'
    sc = 'cg_pool_dgrad_scatter({coef}, {i}, {w}, {b}, {n}, {cin}, {c}, {dx}, (void*)0)'
    good = dict(x='f', b='2L', n='3L', cin='8', wp='f', c='32', ws='f', z='f', i='k', w='f', xbar='f', out='f', coef='f', t='f', dx='f', s='f', vin='f', mean='f', var='f')
    null, inull, odd = '(float*)0', '(int*)0', '(f + 1)'       # the host array stands in for device memory: nothing may be launched
    counts = (dict(b='0L'), dict(n='0L'), dict(b='1L', n='1L'), dict(b='4097L', n='4096L'), dict(b='16777217L', n='1L'), dict(cin='0'), dict(c='-32'))
    widths = (dict(cin='4'), dict(cin='12'), dict(cin='136'), dict(c='16'), dict(c='48'), dict(c='1056'))
    cases = [(call, b, 'CG_ERR_ARG') for call in (ex, st, va, ga, sc) for b in counts]
    cases += [(call, b, 'CG_ERR_UNSUPPORTED') for call in (ex, st, va, ga, sc) for b in widths]
    cases += [(call, dict(b='0L', cin='12'), 'CG_ERR_ARG') for call in (ex, st, va, ga, sc)]          # the counts are judged before the widths
    cases += [(ex, b, 'CG_ERR_ARG') for b in (dict(x=null), dict(wp=null), dict(ws=null), dict(z=null), dict(i=inull), dict(x=odd), dict(wp=odd))]
    cases += [(st, b, 'CG_ERR_ARG') for b in (dict(w=null), dict(xbar=null), dict(mean=null), dict(z=null), dict(out=null), dict(s=null, z=null),
                                             dict(vin=null, out=null))]
    cases += [(va, b, 'CG_ERR_ARG') for b in (dict(x=null), dict(wp=null), dict(mean=null), dict(ws=null), dict(var=null), dict(x=odd), dict(wp=odd))]
    cases += [(ga, b, 'CG_ERR_ARG') for b in (dict(x=null), dict(coef=null), dict(i=inull), dict(t=null))]
    cases += [(sc, b, 'CG_ERR_ARG') for b in (dict(coef=null), dict(i=inull), dict(w=null), dict(dx=null))]
    body = ''.join(f'  bad += {call.format(**{**good, **b})} != {want};   /* {b} */\n' for call, b, want in cases)
    for b, n, c, want in ((2, 1, 32, 256), (1, 1024, 32, 128), (1, 1025, 32, 256), (3, 1025, 96, 4 * 3 * 2 * 96), (34, 8192, 1024, 4 * 34 * 8 * 1024),
                          (1, 16777216, 1024, 4 * 16384 * 1024)):
        body += f'  bad += cg_pool_extrema_workspace({b}L, {n}L, {c}) != {want}L;\n'
    for b, n, c, want in ((2, 1, 32, 64), (1, 1025, 32, 64), (34, 8192, 1024, 34 * 8 * 1024)):
        body += f'  bad += cg_pool_var_workspace({b}L, {n}L, {c}) != {want}L;\n'
    body += '  bad += cg_pool_var_workspace(2L, 3L, 48) != CG_ERR_UNSUPPORTED;\n  bad += cg_pool_var_workspace(1L, 1L, 32) != CG_ERR_ARG;\n'
    body += ('  bad += cg_pool_extrema_workspace(2L, 3L, 48) != CG_ERR_UNSUPPORTED;\n  bad += cg_pool_extrema_workspace(1L, 1L, 32) != CG_ERR_ARG;\n'
             '  bad += cg_pool_extrema_workspace(0L, 3L, 48) != CG_ERR_ARG;\n')
    for k, order in enumerate((HEADERS, HEADERS[::-1])):
        src = (''.join(f'#include "{h}"\n' for h in order) + '#include "catgrasp_amd_pool.h"\n#include <stdio.h>\n'
               'typedef void (*fn_t)(void);\nint main(void) {\n  fn_t table[] = {\n' + ''.join(f'    (fn_t)&{s},\n' for s in SYMBOLS)
               + '  };\n  float f[8];\n  int k[4];\n  int bad = 0;\n  f[0] = 0.f;\n  k[0] = 0;\n' + body
               + '  printf("%d %d %d %d\\n", (int)(sizeof table / sizeof table[0]), CG_POOL_ROWS, CG_POOL_MAX_CIN, CG_POOL_MAX_C);\n  return bad;\n}\n')
        (tmp_path / f'main{k}.c').write_text(src)
        libdir = os.path.dirname(_lib.LIB_PATH)
        subprocess.check_call(GCC + [f'main{k}.c', '-L', libdir, '-lcatgrasp_amd', f'-Wl,-rpath,{libdir}', '-Wl,--allow-shlib-undefined', '-o', f'main{k}'],
                              cwd=tmp_path)
        out = subprocess.run([str(tmp_path / f'main{k}')], capture_output=True, text=True)
        assert out.returncode == 0, (out.returncode, out.stdout, out.stderr)
        assert out.stdout.split() == [str(len(SYMBOLS)), '1024', '128', '1024']
    (tmp_path / 'alone.c').write_text('#include "catgrasp_amd_pool.h"\nint main(void) { return CG_OK; }\n')
    subprocess.check_call(GCC + ['-fsyntax-only', 'alone.c'], cwd=tmp_path)


def test_symbols_are_the_headers_own_and_the_binding_takes_its_types_from_it():
    for name in OTHERS:
        assert not set(SYMBOLS) & set(getattr(_lib, name)()), name
    assert len(_lib.declared_symbols()) == 71
    lib = _lib.lib()
    vp, ci, cl, cf = ctypes.c_void_p, ctypes.c_int, ctypes.c_long, ctypes.c_float
    assert lib.cg_pool_extrema_workspace.restype is cl and tuple(lib.cg_pool_extrema_workspace.argtypes) == (cl, cl, ci)
    assert lib.cg_pool_extrema.restype is ci and tuple(lib.cg_pool_extrema.argtypes) == (vp, cl, cl, ci, vp, vp, ci, vp, vp, vp, vp, vp)
    assert tuple(lib.cg_pool_stats.argtypes) == (vp,) * 7 + (cf, cl, cl, ci, ci, vp, ci) + (vp,) * 7
    assert lib.cg_pool_var_workspace.restype is cl and tuple(lib.cg_pool_var.argtypes) == (vp, cl, cl, ci, vp, vp, ci, vp, vp, vp, vp)
    assert [lib.cg_pool_var_workspace(b, n, c) for b, n, c in ((2, 3, 32), (2, 1025, 32), (2, 3, 48), (1, 1, 32))] == [64, 128, -2, -1]
    assert lib.cg_pool_var(None, 2, 3, 8, None, None, 32, None, None, None, None) == -1
    assert tuple(lib.cg_pool_wgrad_gather.argtypes) == (vp, cl, cl, ci, vp, vp, ci, vp, vp)
    assert tuple(lib.cg_pool_dgrad_scatter.argtypes) == (vp, vp, vp, cl, cl, ci, ci, vp, vp)
    with pytest.raises(ctypes.ArgumentError):
        lib.cg_pool_extrema_workspace(2, 3, 32.0)
    assert [lib.cg_pool_extrema_workspace(b, n, c) for b, n, c in ((2, 3, 32), (2, 1025, 32), (2, 3, 48), (1, 1, 32))] == [256, 512, -2, -1]
    assert lib.cg_pool_extrema(None, 2, 3, 8, None, None, 32, None, None, None, None, None) == -1
    assert lib.cg_pool_extrema(None, 2, 3, 12, None, None, 32, None, None, None, None, None) == -2
    assert lib.cg_pool_wgrad_gather(None, 2, 3, 8, None, None, 32, None, None) == -1
    assert lib.cg_pool_dgrad_scatter(None, None, None, 2, 3, 8, 48, None, None) == -2


def test_lib_raises_when_the_library_lacks_a_pool_symbol(monkeypatch):
    real = _lib.pool_signatures()
    monkeypatch.setattr(_lib, '_lib', None)
    monkeypatch.setattr(_lib, 'pool_signatures', lambda: {**real, 'cg_pool_not_built': (ctypes.c_int, ())})
    with pytest.raises(_lib.CatgraspAmdError, match='cg_pool_not_built'):
        _lib.lib()


def test_build_tracks_the_pool_header_and_compiles_the_kernels():
    from catgrasp_amd import build
    assert 'catgrasp_amd_pool.h' in inspect.getsource(build.build)
    src = [s for s in build.sources() if s.endswith('pool_train.hip')]
    assert len(src) == 1
    with open(src[0]) as f:
        text = f.read()
    assert 'catgrasp_amd_pool.h' in text and 'fmaf(' in text and 'mfma32(' in text and 'atomic' not in text and 'asm' not in text


def test_the_pool_kernels_stay_out_of_scratch_and_leave_room_for_two_workgroups():
    """Code-object metadata of the built gfx950 image (scripts/kernel_resources.py; no GPU needed): no private segment, no spilled
    registers in any kernel of pool_train.hip; both forms of the tile kernel take at most 128 of a SIMD's 512 registers per lane (vector
    and accumulator together) and at most a quarter of a CU's 160 KB of LDS: four workgroups of four waves fit a CU."""
    import importlib.util
    spec = importlib.util.spec_from_file_location('kernel_resources', os.path.join(ROOT, 'scripts', 'kernel_resources.py'))
    kr = importlib.util.module_from_spec(spec); spec.loader.exec_module(kr)
    if not all(os.path.exists(os.path.join(kr.LLVM, t)) for t in ('llvm-objcopy', 'clang-offload-bundler', 'llvm-readelf')) or shutil.which('c++filt') is None:
        pytest.skip('ROCm llvm binutils / c++filt not found')
    path = os.path.join(ROOT, 'catgrasp_amd', 'csrc', 'pool_train.o')
    if not os.path.exists(path):
        pytest.skip('pool_train.o not built')
    seen = {}
    for r in kr.resources(path):
        seen[r['kernel'].replace('void ', '')] = r
        assert r['private_segment_fixed_size'] == 0 and r['vgpr_spill_count'] == 0 and r['sgpr_spill_count'] == 0, r
    assert sorted(seen) == ['pool_extrema_kernel<false>', 'pool_extrema_kernel<true>', 'pool_gather_kernel', 'pool_scatter_kernel', 'pool_select_kernel',
                            'pool_stats_kernel', 'pool_var_total_kernel'], sorted(seen)
    for name in ('pool_extrema_kernel<false>', 'pool_extrema_kernel<true>'):
        ex = seen[name]
        assert ex['vgpr_count'] + ex['agpr_count'] <= 128 and ex['group_segment_fixed_size'] <= 40 * 1024, ex


def test_the_wrappers_refuse_host_tensors_before_any_device_work(monkeypatch):
    class FakeLib:
        def __getattr__(self, name):
            raise AssertionError(f'{name} was reached')
    monkeypatch.setattr(_lib, 'lib', lambda: FakeLib())
    x, w, v = torch.zeros(2, 5, 8), torch.zeros(32, 8), torch.zeros(32)
    i = torch.zeros((2, 32), dtype=torch.int32)
    for fn, args in ((PA.pool_extrema, (x, w, v, v)), (PA.pool_stats, (w, v, torch.zeros(8), torch.zeros(8, 8), v, v, 1e-5, 5, torch.zeros(2, 32), True)),
                     (PA.pool_var, (x, w, v, v)), (PA.pool_mean, (w, v, torch.zeros(8), 2, 5)),
                     (PA.pool_wgrad_gather, (x, torch.zeros(2, 32), i)), (PA.pool_dgrad_scatter, (x, torch.zeros(2, 32), i, w))):
        with pytest.raises(NotImplementedError, match='HIP device'):
            fn(*args)
    with pytest.raises(NotImplementedError, match='float32'):
        PA.pool_extrema(x.double(), w)
    with pytest.raises(ValueError, match='contiguous'):
        PA.pool_extrema(x.transpose(0, 1), w)
    with pytest.raises(ValueError, match='kernel size 1'):
        PA.rows_layer(torch.zeros(4, 8), nn.Conv1d(8, 32, 3), nn.BatchNorm1d(32))
    conv, bn = nn.Conv1d(8, 32, 1), nn.BatchNorm1d(32).train()
    with pytest.raises(NotImplementedError, match='HIP device'):
        PA.conv_bn_max_train(x, conv, bn, True)
    with pytest.raises(NotImplementedError, match='float32'):
        PA.conv_bn_max_train(x.double(), conv.double(), bn.double(), True)
    with pytest.raises(ValueError, match='training mode'):
        PA.conv_bn_max_train(x, conv, nn.BatchNorm1d(32).eval(), True)
    with pytest.raises(ValueError, match='kernel size 1'):
        PA.conv_bn_max_train(x, nn.Conv1d(8, 32, 3), bn, True)
    assert int(bn.num_batches_tracked) == 0
    assert pointnet2_train.ENCODER_ON_HIP is False and pointnet2_train.USE_TORCH_OPS is False
    monkeypatch.setattr(pointnet2_train, 'ENCODER_ON_HIP', True)
    model = pointnet2_train.PointNetSeg(6, 12).train()
    with pytest.raises(NotImplementedError, match='HIP device'):
        model(torch.zeros(2, 8, 6))
