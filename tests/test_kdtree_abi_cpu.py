"""CPU tests (no GPU) of the boundary of the k-d tree searches: include/catgrasp_amd_kdtree.h is plain C99 next to the other six headers
and links from C, every argument error comes back without a GPU, the ctypes binding takes its types from that header, lib() requires its
symbols, the build tracks it, and the Python front refuses what it does not do before any device work."""
import ctypes
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from catgrasp_amd import _lib, neighbors

INCLUDE = os.path.dirname(_lib.KDTREE_HEADER_PATH)
KDTREE_SYMBOLS = ['cg_grid_ball_fill', 'cg_grid_nearest']
HEADERS = ['catgrasp_amd.h', 'catgrasp_amd_cluster.h', 'catgrasp_amd_sparse.h', 'catgrasp_amd_pointgroup.h', 'catgrasp_amd_scene.h',
           'catgrasp_amd_neighbors.h', 'catgrasp_amd_kdtree.h']


def test_kdtree_header_is_strict_c99_with_the_other_six_in_either_order_and_links_from_c(tmp_path):
    if shutil.which('gcc') is None:
        pytest.fail('gcc is needed to check the header')
    assert sorted(_lib.kdtree_signatures()) == KDTREE_SYMBOLS
    grid = '{pts}, {idx}, {keys}, {n}, {ox}, 0.0, 0.5, {cell}, {ex}, 60L, 50L, {q}, {f64}, {order}, {m}'
    nearest = 'cg_grid_nearest(' + grid + ', {oi}, {od}, {rounds}, (void*)0)'
    fill = 'cg_grid_ball_fill(' + grid + ', {r}, {off}, {total}, {oi}, (void*)0)'
    good = dict(pts='d', idx='i', keys='k', n='16L', ox='0.0', cell='0.002', ex='1300L', q='f', f64=0, order='i', m='4L', oi='i', od='d',
                rounds='i', r='0.002', off='k', total='7L')
    # the host arrays stand in for device memory: nothing may be launched, so nothing reads them
    bad_common = [dict(pts='(double*)0'), dict(idx='(int*)0'), dict(keys='(long long*)0'), dict(n='0L'), dict(n='-3L'), dict(ox='1.0 / zero'),
                  dict(ox='zero / zero'), dict(cell='0.0'), dict(cell='-0.002'), dict(cell='1.0 / zero'), dict(cell='zero / zero'), dict(ex='0L'),
                  dict(ex='1L << 52'),                                                     # 2^52 * 3000 >= 2^62
                  dict(q='(float*)0'), dict(q='(double*)0', f64=1), dict(m='0L'), dict(m='-1L'), dict(oi='(int*)0')]
    bad = {nearest: bad_common + [dict(od='(double*)0'), dict(od='(double*)0', rounds='(int*)0')],
           fill: bad_common + [dict(r='0.0'), dict(r='-0.002'), dict(r='1.0 / zero'), dict(r='zero / zero'), dict(r='0.0020001'),   # beyond the cell
                               dict(r='1e-160', cell='1e-160'),                             # r * r is no normal number
                               dict(off='(long long*)0'), dict(total='-1L'), dict(off='(long long*)0', total='0L', oi='(int*)0')]}
    body = ''.join('  bad += ' + call.format(**{**good, **b}) + f' != CG_ERR_ARG;   /* {b} */\n' for call, cases in bad.items() for b in cases)
    too_many = str(2 ** 31) + 'L'
    for call in (nearest, fill):
        for b in (dict(n=too_many), dict(m=too_many)):
            body += '  bad += ' + call.format(**{**good, **b}) + ' != CG_ERR_UNSUPPORTED;\n'
    # a total of zero needs no indices and launches nothing; NULL rounds is taken (the complaint is the NULL table)
    body += '  bad += ' + fill.format(**{**good, 'total': '0L', 'oi': '(int*)0'}) + ' != CG_OK;\n'
    body += '  bad += ' + nearest.format(**{**good, 'rounds': '(int*)0', 'pts': '(double*)0'}) + ' != CG_ERR_ARG;\n'
    for n, order in enumerate((HEADERS, HEADERS[::-1])):
        src = (''.join(f'#include "{h}"\n' for h in order) + '#include "catgrasp_amd_kdtree.h"\n#include <stdio.h>\n'
               'typedef void (*fn_t)(void);\nint main(void) {\n  fn_t table[] = {\n' + ''.join(f'    (fn_t)&{s},\n' for s in KDTREE_SYMBOLS)
               + '  };\n  double d[48]; float f[12]; int i[16]; long long k[16]; volatile double zero = 0.0;\n  int bad = 0;\n'
               '  d[0] = 0.0; f[0] = 0.f; i[0] = 0; k[0] = 0;\n' + body
               + '  printf("%d %d\\n", (int)(sizeof table / sizeof table[0]), CG_KD_MAX_ROUNDS);\n  return bad;\n}\n')
        (tmp_path / f'main{n}.c').write_text(src)
        libdir = os.path.dirname(_lib.LIB_PATH)
        subprocess.check_call(['gcc', '-std=c99', '-Wall', '-Wextra', '-Werror', '-pedantic', '-I', INCLUDE, f'main{n}.c', '-L', libdir,
                               '-lcatgrasp_amd', f'-Wl,-rpath,{libdir}', '-Wl,--allow-shlib-undefined', '-o', f'main{n}'], cwd=tmp_path)
        out = subprocess.run([str(tmp_path / f'main{n}')], capture_output=True, text=True)
        assert out.returncode == 0, (out.returncode, out.stdout, out.stderr)
        rounds_cap = int(out.stdout.split()[1])
        assert out.stdout.split()[0] == '2' and 1 <= rounds_cap <= 64


def test_binding_takes_the_kdtree_types_from_the_header_and_leaves_the_other_headers_alone():
    lib = _lib.lib()
    vp, ci, cl, cd = ctypes.c_void_p, ctypes.c_int, ctypes.c_long, ctypes.c_double
    with open(_lib.KDTREE_HEADER_PATH) as f:
        text = re.sub(r'/\*.*?\*/', '', f.read(), flags=re.S)
    for name in KDTREE_SYMBOLS:
        m = re.search(r'\bint\s+' + name + r'\s*\(([^)]*)\)\s*;', text)
        params = [' '.join(q.split()) for q in m.group(1).split(',')]
        fn = getattr(lib, name)
        assert fn.restype is ci and len(fn.argtypes) == len(params), name
        for at, q in zip(fn.argtypes, params):
            assert at is (vp if '*' in q else {'int': ci, 'long': cl, 'double': cd}[q.rsplit(' ', 1)[0]]), (name, q)
    grid = (vp, vp, vp, cl, cd, cd, cd, cd, cl, cl, cl)
    assert tuple(lib.cg_grid_nearest.argtypes) == grid + (vp, ci, vp, cl, vp, vp, vp, vp)
    assert tuple(lib.cg_grid_ball_fill.argtypes) == grid + (vp, ci, vp, cl, cd, vp, cl, vp, vp)
    g = (None, None, None, 16, 0.0, 0.0, 0.0, 0.002, 4, 4, 4)
    with pytest.raises(ctypes.ArgumentError):
        lib.cg_grid_nearest(*g, None, 0.5, None, 4, None, None, None, None)
    with pytest.raises(ctypes.ArgumentError):
        lib.cg_grid_ball_fill(*g, None, 0, None, 4, 0.002, None, 7.0, None, None)
    assert lib.cg_grid_nearest(*g, None, 0, None, 4, None, None, None, None) == -1
    assert lib.cg_grid_ball_fill(*g, None, 0, None, 4, 0.002, None, 0, None, None) == -1
    assert lib.cg_grid_nearest(*g, None, 0, None, 2 ** 31 + 5, None, None, None, None) == -1     # a long arrives intact; NULL comes first
    # the other headers' views are unchanged
    assert len(_lib.declared_symbols()) == 71
    assert sorted(_lib.neighbors_signatures()) == ['cg_grid_cell_keys', 'cg_grid_count_within', 'cg_grid_nearest_within', 'cg_grid_normals']
    for sigs in (_lib.signatures(), _lib.cluster_signatures(), _lib.sparse_signatures(), _lib.pointgroup_signatures(), _lib.scene_signatures(),
                 _lib.neighbors_signatures()):
        assert not set(KDTREE_SYMBOLS) & set(sigs)


def test_lib_raises_when_the_library_lacks_a_kdtree_symbol(monkeypatch):
    real = _lib.kdtree_signatures()
    monkeypatch.setattr(_lib, '_lib', None)
    monkeypatch.setattr(_lib, 'kdtree_signatures', lambda: {**real, 'cg_grid_not_built': (ctypes.c_int, ())})
    with pytest.raises(_lib.CatgraspAmdError, match='cg_grid_not_built'):
        _lib.lib()


def test_build_tracks_the_kdtree_header_and_the_kernels_share_the_grid_code():
    from catgrasp_amd import build
    assert 'catgrasp_amd_kdtree.h' in inspect.getsource(build.build)
    src = [s for s in build.sources() if s.endswith('grid_index.hip')]
    assert len(src) == 1
    with open(src[0]) as f:
        text = f.read()
    assert '#include "cg_normals.hpp"' in text and 'catgrasp_amd_kdtree.h' in text
    assert text.count('cell_range(double q') == 1 and 'asm' not in re.sub(r'//.*', '', text)       # one text of the lemma; no inline assembly
    assert 'seven' in _lib.__doc__


class _NoDeviceIndex:
    """Stands where GridIndex would: a tree whose every device call is an error."""
    cell = 0.002

    def __init__(self, points, cell, device=None):
        self.n, self.device = len(points), None

    def __getattr__(self, name):
        raise AssertionError(f'device work ({name}) before the refusal')


def test_python_refusals_come_before_any_device_work(monkeypatch):
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    P = np.random.default_rng(0).uniform(0, 0.01, (50, 3)).astype(np.float32)
    # without a HIP device nothing is built, not even for empty data
    for fn in (lambda: neighbors.cKDTree(P), lambda: neighbors.cKDTree(torch.from_numpy(P)), lambda: neighbors.cKDTree(P, device='cpu'),
               lambda: neighbors.cKDTree(P[:0]), lambda: neighbors.cKDTree(P, cell=0.002)):
        with pytest.raises(_lib.CatgraspAmdError, match='HIP device'):
            fn()
    # bad data is refused before the device is asked for
    for bad in (np.nan, np.inf, -np.inf):
        Q = P.copy()
        Q[17, 1] = bad
        with pytest.raises(ValueError, match='NaN or infinity'):
            neighbors.cKDTree(Q)
        with pytest.raises(ValueError, match='NaN or infinity'):
            neighbors.cKDTree(Q.astype(np.float64), cell=0.002)
    for shape in ((50, 2), (150,), (5, 10, 3)):
        with pytest.raises(ValueError, match='shape'):
            neighbors.cKDTree(P.reshape(-1)[:int(np.prod(shape))].reshape(shape))
    for c in (0.0, -0.002, float('inf'), float('nan'), '0.002', True):
        with pytest.raises(ValueError, match='cell'):
            neighbors.cKDTree(P, cell=c)
    # the queries of a tree: every refusal fires before the index is touched
    monkeypatch.setattr(neighbors, 'GridIndex', _NoDeviceIndex)
    tree = neighbors.cKDTree(P)
    assert tree.n == 50 and tree.m == 3 and np.array_equal(tree.data, P)
    for kw in (dict(k=2), dict(k=[1]), dict(k=0), dict(p=1), dict(p=np.inf), dict(eps=0.1)):
        with pytest.raises(NotImplementedError, match='reference'):
            tree.query(P[:3], **kw)
    for kw in (dict(p=1), dict(eps=0.5)):
        with pytest.raises(NotImplementedError, match='reference'):
            tree.query_ball_point(P[:3], 0.002, **kw)
    for bad in (np.nan, np.inf, -np.inf):
        Q = P[:4].astype(np.float64)
        Q[2, 0] = bad
        for fn in (lambda: tree.query(Q), lambda: tree.query(Q[2]), lambda: tree.query_ball_point(Q, 0.002),
                   lambda: tree.query_ball_point(Q, 0.002, return_length=True)):
            with pytest.raises(ValueError, match='NaN or infinity'):
                fn()
    for x in (P[:4, :2], P[0, :2], np.zeros((2, 2, 3)), np.zeros(4)):
        with pytest.raises(ValueError, match='shape'):
            tree.query(x)
        with pytest.raises(ValueError, match='shape'):
            tree.query_ball_point(x, 0.002)
    for r in (0.0, -0.002, float('inf'), float('nan'), None):
        with pytest.raises(ValueError, match='r must be'):
            tree.query_ball_point(P[:3], r)
    for b in (-1.0, float('nan')):
        with pytest.raises(ValueError, match='distance_upper_bound'):
            tree.query(P[:3], distance_upper_bound=b)


def test_the_default_cell_holds_a_few_points_and_is_never_degenerate():
    # a filled box, a sheet in it, a line, a point: about 4 points per occupied cell, by the rule of the docstring
    assert neighbors.default_cell((0, 0, 0), (1, 1, 1), 4000) == pytest.approx(0.1)
    assert neighbors.default_cell((0, 0, 0), (1, 0, 1), 40000) == pytest.approx(0.01)
    assert neighbors.default_cell((0, 5, 0), (0, 7, 0), 8) == pytest.approx(1.0)
    assert neighbors.default_cell((3, 3, 3), (3, 3, 3), 100) == 1.0
    assert neighbors.default_cell((0, 0, 0), (1e-200, 0, 0), 2) == 1.0
