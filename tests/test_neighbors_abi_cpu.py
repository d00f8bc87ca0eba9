"""CPU tests (no GPU) of the grid index's boundary: include/catgrasp_amd_neighbors.h is plain C99 next to the other five headers and links
from C, argument errors and the max_nn limit come back without a GPU, the ctypes binding takes its types from that header, lib() requires
its symbols, the other headers keep their symbol sets, and the Python front refuses what it cannot do and refuses to run without a HIP
device."""
import ctypes
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from catgrasp_amd import _lib, neighbors, scene

INCLUDE = os.path.dirname(_lib.NEIGHBORS_HEADER_PATH)
NEIGHBORS_SYMBOLS = ['cg_grid_cell_keys', 'cg_grid_count_within', 'cg_grid_nearest_within', 'cg_grid_normals']
HEADERS = ['catgrasp_amd.h', 'catgrasp_amd_cluster.h', 'catgrasp_amd_sparse.h', 'catgrasp_amd_pointgroup.h', 'catgrasp_amd_scene.h',
           'catgrasp_amd_neighbors.h']


def _compile_and_run(tmp_path, name, src):
    (tmp_path / f'{name}.c').write_text(src)
    libdir = os.path.dirname(_lib.LIB_PATH)
    subprocess.check_call(['gcc', '-std=c99', '-Wall', '-Wextra', '-Werror', '-pedantic', '-I', INCLUDE, f'{name}.c', '-L', libdir, '-lcatgrasp_amd',
                           f'-Wl,-rpath,{libdir}', '-Wl,--allow-shlib-undefined', '-o', name], cwd=tmp_path)
    return subprocess.run([str(tmp_path / name)], capture_output=True, text=True)


def test_neighbors_header_is_strict_c99_with_the_other_five_in_either_order_and_links_from_c(tmp_path):
    if shutil.which('gcc') is None:
        pytest.fail('gcc is needed to check the header')
    syms = sorted(_lib.neighbors_signatures())
    assert syms == NEIGHBORS_SYMBOLS
    grid = '{pts}, {idx}, {keys}, {n}, {ox}, 0.0, 0.5, {cell}, {ex}, 60L, 50L'
    normals = 'cg_grid_normals(' + grid + ', {r}, {nn}, 0.0, 0.0, {vz}, {out}, (int*)0, (double*)0, (void*)0)'
    nearest = 'cg_grid_nearest_within(' + grid + ', {q}, 0, {order}, {m}, {r}, {oi}, {out}, (void*)0)'
    count = 'cg_grid_count_within(' + grid + ', {q}, 1, {order}, {m}, {r}, {oi}, (void*)0)'
    keys = 'cg_grid_cell_keys({q}, 0, {n}, {ox}, 0.0, 0.5, {cell}, {ex}, 60L, 50L, {keys}, (void*)0)'
    good = dict(pts='d', idx='i', keys='k', n='16L', ox='0.0', cell='0.002', ex='1300L', r='0.002', nn=30, vz='0.0', out='d', q='f', order='i',
                m='4L', oi='i')
    # the host arrays stand in for device memory: nothing may be launched, so nothing reads them
    bad_grid = [dict(pts='(double*)0'), dict(idx='(int*)0'), dict(keys='(long long*)0'), dict(n='0L'), dict(n='-3L'), dict(ox='1.0 / zero'),
                dict(cell='0.0'), dict(cell='-0.002'), dict(cell='1.0 / zero'), dict(ex='0L'), dict(ex='1L << 52'),      # 2^52 * 3000 >= 2^62
                dict(r='0.0'), dict(r='-0.002'), dict(r='1.0 / zero'), dict(r='zero / zero'), dict(r='0.0020001'),      # beyond the cell
                dict(r='1e-160', cell='1e-160')]                                                                         # r * r is no normal number
    bad = {normals: bad_grid + [dict(nn=0), dict(nn=-1), dict(vz='1.0 / zero'), dict(out='(double*)0')],
           nearest: bad_grid + [dict(q='(float*)0'), dict(m='0L'), dict(oi='(int*)0'), dict(out='(double*)0')],
           count: bad_grid + [dict(q='(double*)0'), dict(m='-1L'), dict(oi='(int*)0')],
           keys: [dict(q='(float*)0'), dict(keys='(long long*)0'), dict(n='0L'), dict(cell='0.0'), dict(ex='0L'), dict(ex='1L << 52'),
                  dict(ox='zero / zero')]}
    body = ''.join('  bad += ' + call.format(**{**good, **b}) + f' != CG_ERR_ARG;   /* {b} */\n' for call, cases in bad.items() for b in cases)
    # the contract limit: with and without device pointers, and before any other complaint
    body += '  bad += ' + normals.format(**{**good, 'nn': 65}) + ' != CG_ERR_UNSUPPORTED;\n'
    body += '  bad += ' + normals.format(**{**good, 'nn': 65, 'pts': '(double*)0', 'idx': '(int*)0', 'keys': '(long long*)0', 'out': '(double*)0'}) \
        + ' != CG_ERR_UNSUPPORTED;\n'
    body += '  bad += ' + normals.format(**{**good, 'nn': 'CG_NB_MAX_NN + 1'}) + ' != CG_ERR_UNSUPPORTED;\n'
    body += '  bad += ' + normals.format(**{**good, 'nn': 'CG_NB_MAX_NN', 'pts': '(double*)0'}) + ' != CG_ERR_ARG;   /* 64 itself is taken */\n'
    for n, order in enumerate((HEADERS, HEADERS[::-1])):
        src = (''.join(f'#include "{h}"\n' for h in order) + '#include "catgrasp_amd_neighbors.h"\n#include <stdio.h>\n'
               'typedef void (*fn_t)(void);\nint main(void) {\n  fn_t table[] = {\n' + ''.join(f'    (fn_t)&{s},\n' for s in syms) + '  };\n'
               '  double d[48]; float f[12]; int i[16]; long long k[16]; volatile double zero = 0.0;\n  int bad = 0;\n'
               '  d[0] = 0.0; f[0] = 0.f; i[0] = 0; k[0] = 0;\n' + body
               + '  printf("%d %d\\n", (int)(sizeof table / sizeof table[0]), CG_NB_MAX_NN);\n  return bad;\n}\n')
        out = _compile_and_run(tmp_path, f'main{n}', src)
        assert out.returncode == 0, (out.returncode, out.stdout, out.stderr)
        assert out.stdout.split() == ['4', '64']


def test_binding_takes_the_neighbors_types_from_the_header_and_leaves_the_other_headers_alone():
    lib = _lib.lib()
    vp, ci, cl, cd = ctypes.c_void_p, ctypes.c_int, ctypes.c_long, ctypes.c_double
    with open(_lib.NEIGHBORS_HEADER_PATH) as f:
        text = re.sub(r'/\*.*?\*/', '', f.read(), flags=re.S)
    for name in NEIGHBORS_SYMBOLS:
        m = re.search(r'\bint\s+' + name + r'\s*\(([^)]*)\)\s*;', text)
        params = [' '.join(q.split()) for q in m.group(1).split(',')]
        fn = getattr(lib, name)
        assert fn.restype is ci and len(fn.argtypes) == len(params), name
        for at, q in zip(fn.argtypes, params):
            assert at is (vp if '*' in q else {'int': ci, 'long': cl, 'double': cd}[q.rsplit(' ', 1)[0]]), (name, q)
    grid = (vp, vp, vp, cl, cd, cd, cd, cd, cl, cl, cl)
    assert tuple(lib.cg_grid_cell_keys.argtypes) == (vp, ci, cl, cd, cd, cd, cd, cl, cl, cl, vp, vp)
    assert tuple(lib.cg_grid_normals.argtypes) == grid + (cd, ci, cd, cd, cd, vp, vp, vp, vp)
    assert tuple(lib.cg_grid_nearest_within.argtypes) == grid + (vp, ci, vp, cl, cd, vp, vp, vp)
    assert tuple(lib.cg_grid_count_within.argtypes) == grid + (vp, ci, vp, cl, cd, vp, vp)
    g = (None, None, None, 16, 0.0, 0.0, 0.0, 0.002, 4, 4, 4)
    with pytest.raises(ctypes.ArgumentError):
        lib.cg_grid_normals(*g, 0.002, 30.5, 0.0, 0.0, 0.0, None, None, None, None)
    with pytest.raises(ctypes.ArgumentError):
        lib.cg_grid_count_within(None, None, None, 16.0, *g[4:], None, 0, None, 4, 0.002, None, None)
    assert lib.cg_grid_normals(*g, 0.002, 30, 0.0, 0.0, 0.0, None, None, None, None) == -1
    assert lib.cg_grid_normals(*g, 0.002, 65, 0.0, 0.0, 0.0, None, None, None, None) == -2
    assert lib.cg_grid_nearest_within(*g, None, 0, None, 4, 0.002, None, None, None) == -1
    assert lib.cg_grid_count_within(*g, None, 0, None, 4, 0.002, None, None) == -1
    assert lib.cg_grid_cell_keys(None, 0, 2 ** 31 + 5, 0.0, 0.0, 0.0, 0.002, 4, 4, 4, None, None) == -1     # a long arrives intact, and is refused
    # the other headers' views are unchanged
    assert len(_lib.declared_symbols()) == 71
    for sigs in (_lib.signatures(), _lib.cluster_signatures(), _lib.sparse_signatures(), _lib.pointgroup_signatures(), _lib.scene_signatures()):
        assert not set(NEIGHBORS_SYMBOLS) & set(sigs)
    assert sorted(_lib.scene_signatures()) == ['cg_depth_to_xyz', 'cg_organized_normals', 'cg_scene_halo_fits']
    assert sorted(_lib.cluster_signatures()) == ['cg_meanshift_climb', 'cg_meanshift_lds_max_points', 'cg_meanshift_merge']
    assert sorted(_lib.sparse_signatures()) == ['cg_sparse_conv', 'cg_sparse_keys', 'cg_sparse_rules_down', 'cg_sparse_rules_inverse', 'cg_sparse_rules_subm']
    assert sorted(_lib.pointgroup_signatures()) == ['cg_sparse_conv_cat']


def test_lib_raises_when_the_library_lacks_a_neighbors_symbol(monkeypatch):
    real = _lib.neighbors_signatures()
    monkeypatch.setattr(_lib, '_lib', None)
    monkeypatch.setattr(_lib, 'neighbors_signatures', lambda: {**real, 'cg_grid_not_built': (ctypes.c_int, ())})
    with pytest.raises(_lib.CatgraspAmdError, match='cg_grid_not_built'):
        _lib.lib()


def test_build_tracks_the_neighbors_header_and_the_shared_normals_header():
    from catgrasp_amd import build
    assert 'catgrasp_amd_neighbors.h' in inspect.getsource(build.build)
    assert any(s.endswith('grid_index.hip') for s in build.sources())
    csrc = os.path.dirname(build.sources()[0])
    for f in ('scene.hip', 'grid_index.hip'):                              # one text of the arithmetic after the search
        with open(os.path.join(csrc, f)) as fh:
            text = fh.read()
        assert '#include "cg_normals.hpp"' in text and 'jacobi_rotate(double&' not in text


def test_python_refusals_come_before_any_device_work(monkeypatch):
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    P = np.random.default_rng(0).uniform(0, 0.01, (50, 3)).astype(np.float32)
    for bad in (np.nan, np.inf, -np.inf):
        Q = P.copy()
        Q[17, 1] = bad
        for fn in (lambda: neighbors.GridIndex(Q, 0.002), lambda: neighbors.estimate_normals(Q), lambda: neighbors.estimate_normals(Q.astype(np.float64)),
                   lambda: neighbors.cloudA_minus_cloudB(Q, P, 0.005), lambda: neighbors.cloudA_minus_cloudB(torch.from_numpy(P), Q, 0.005)):
            with pytest.raises(ValueError, match='NaN or infinity'):
                fn()
    for c in (0.0, -0.002, float('inf'), float('nan'), None, '0.002', True):
        with pytest.raises(ValueError, match='cell'):
            neighbors.GridIndex(P, c)
        with pytest.raises(ValueError, match='radius'):
            neighbors.estimate_normals(P, radius=c)
        with pytest.raises(ValueError, match='thres'):
            neighbors.cloudA_minus_cloudB(P, P, c)
    for shape in ((50, 2), (150,), (5, 10, 3)):
        with pytest.raises(ValueError, match='shape'):
            neighbors.GridIndex(P.reshape(-1)[:int(np.prod(shape))].reshape(shape), 0.002)
    depth = np.full((8, 9), 0.5, np.float32)
    K = np.array([[2257.75, 0, 40.3], [0, 2257.49, 30.7], [0, 0, 1]])
    for r in (0.0, -0.003, float('inf'), float('nan')):
        with pytest.raises(ValueError, match='radius'):
            scene.scene_from_depth(depth, K, scene_normal_radius=r)
    assert 'scene_normal_radius' in inspect.signature(scene.scene_from_depth).parameters
    assert inspect.signature(scene.scene_from_depth).parameters['scene_normal_radius'].default is None


def test_without_a_hip_device_the_index_raises(monkeypatch):
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)          # on a GPU host too: the refusal, not a CPU fallback
    P = np.random.default_rng(0).uniform(0, 0.01, (50, 3)).astype(np.float32)
    for fn in (lambda: neighbors.GridIndex(P, 0.002), lambda: neighbors.GridIndex(torch.from_numpy(P), 0.002),
               lambda: neighbors.GridIndex(P, 0.002, device='cpu'), lambda: neighbors.GridIndex(P[:0], 0.002),
               lambda: neighbors.estimate_normals(P), lambda: neighbors.estimate_normals(P, device='cpu'),
               lambda: neighbors.cloudA_minus_cloudB(P, P, 0.005)):
        with pytest.raises(_lib.CatgraspAmdError, match='HIP device'):
            fn()
