"""CPU tests (no GPU) of the scene front end's boundary: include/catgrasp_amd_scene.h is plain C99 next to the other four headers and
links from C, argument errors come back without a GPU, the ctypes binding takes its types from that header, lib() requires its
symbols, and the Python front refuses what it cannot do and refuses to run without a HIP device."""
import ctypes
import itertools
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from catgrasp_amd import _lib, pipeline, scene

INCLUDE = os.path.dirname(_lib.SCENE_HEADER_PATH)
SCENE_SYMBOLS = ['cg_depth_to_xyz', 'cg_organized_normals', 'cg_scene_halo_fits']
HEADERS = ['catgrasp_amd.h', 'catgrasp_amd_cluster.h', 'catgrasp_amd_sparse.h', 'catgrasp_amd_pointgroup.h', 'catgrasp_amd_scene.h']
K = np.array([[2257.75, 0, 40.3], [0, 2257.49, 30.7], [0, 0, 1]])


def _compile_and_run(tmp_path, name, src):
    (tmp_path / f'{name}.c').write_text(src)
    libdir = os.path.dirname(_lib.LIB_PATH)
    subprocess.check_call(['gcc', '-std=c99', '-Wall', '-Wextra', '-Werror', '-pedantic', '-I', INCLUDE, f'{name}.c', '-L', libdir, '-lcatgrasp_amd',
                           f'-Wl,-rpath,{libdir}', '-Wl,--allow-shlib-undefined', '-o', name], cwd=tmp_path)
    return subprocess.run([str(tmp_path / name)], capture_output=True, text=True)


def test_scene_header_is_strict_c99_with_the_other_four_in_either_order_and_links_from_c(tmp_path):
    if shutil.which('gcc') is None:
        pytest.fail('gcc is needed to check the header')
    syms = sorted(_lib.scene_signatures())
    assert syms == SCENE_SYMBOLS
    call = ('cg_organized_normals(f, k, {H}, {W}, {fx}, 2257.49, 40.3, 30.7, {r}, {nn}, 0.0, 0.0, {vz}, {route}, {hu}, {hv}, {out}, (int*)0, '
            '(double*)0, (void*)0)')
    good = dict(H=4, W=4, fx='2257.75', r='0.002', nn=30, vz='0.0', route='CG_SCENE_ROUTE_AUTO', hu=9, hv=9, out='d')
    bad = [dict(H=0), dict(W=-1), dict(fx='0.0'), dict(fx='-1.0'), dict(fx='1.0 / zero'), dict(r='0.0'), dict(r='-0.002'), dict(r='1.0 / zero'),
           dict(nn=0), dict(vz='1.0 / zero'), dict(route=3), dict(route=-1), dict(hu=-1), dict(out='(double*)0'),
           dict(route='CG_SCENE_ROUTE_TILED', hu=40, hv=40),                 # a halo beyond the LDS budget, forced
           dict(route='CG_SCENE_ROUTE_TILED', hu=25, hv=24)]
    body = ''.join('  bad += ' + call.format(**{**good, **b}) + f' != CG_ERR_ARG;   /* {b} */\n' for b in bad)
    body += ('  bad += cg_organized_normals((float*)0, k, 4, 4, 2257.75, 2257.49, 40.3, 30.7, 0.002, 30, 0.0, 0.0, 0.0, 0, 9, 9, d, (int*)0, (double*)0, (void*)0) != CG_ERR_ARG;\n'
             '  bad += cg_organized_normals(f, (unsigned char*)0, 4, 4, 2257.75, 2257.49, 40.3, 30.7, 0.002, 30, 0.0, 0.0, 0.0, 0, 9, 9, d, (int*)0, (double*)0, (void*)0) != CG_ERR_ARG;\n'
             '  bad += cg_depth_to_xyz((void*)0, 0, 4, 4, 2257.75, 2257.49, 40.3, 30.7, f, k, (void*)0) != CG_ERR_ARG;\n'
             '  bad += cg_depth_to_xyz(d, 1, 4, 4, 2257.75, 2257.49, 40.3, 30.7, (float*)0, k, (void*)0) != CG_ERR_ARG;\n'
             '  bad += cg_depth_to_xyz(d, 1, 0, 4, 2257.75, 2257.49, 40.3, 30.7, f, k, (void*)0) != CG_ERR_ARG;\n'
             '  bad += cg_depth_to_xyz(d, 1, 4, 4, 2257.75, 0.0, 40.3, 30.7, f, k, (void*)0) != CG_ERR_ARG;\n'
             '  bad += cg_depth_to_xyz(d, 1, 4, 4, 2257.75, 2257.49, 1.0 / zero, 30.7, f, k, (void*)0) != CG_ERR_ARG;\n')
    # the budget as the header states it: (tile + 2 halo_u) * (tile + 2 halo_v) staged pixels of 16 bytes within CG_SCENE_LDS_BUDGET
    fits = ('  printf("%d %d %d %d %d %d %d %d\\n", (int)(sizeof table / sizeof table[0]), CG_SCENE_TILE, CG_SCENE_LDS_BUDGET, cg_scene_halo_fits(24, 24), '
            'cg_scene_halo_fits(25, 24), cg_scene_halo_fits(0, 120), cg_scene_halo_fits(0, 121), cg_scene_halo_fits(-1, 2));\n')
    for n, order in enumerate((HEADERS, HEADERS[::-1])):
        src = (''.join(f'#include "{h}"\n' for h in order) + '#include "catgrasp_amd_scene.h"\n#include <stdio.h>\n'
               'typedef void (*fn_t)(void);\nint main(void) {\n  fn_t table[] = {\n' + ''.join(f'    (fn_t)&{s},\n' for s in syms) + '  };\n'
               '  double d[16]; float f[48]; unsigned char k[16]; volatile double zero = 0.0;\n  int bad = 0;\n  d[0] = 0.0; f[0] = 0.f; k[0] = 0;\n'
               + body + fits + '  return bad;\n}\n')
        out = _compile_and_run(tmp_path, f'main{n}', src)
        assert out.returncode == 0, (out.returncode, out.stdout, out.stderr)
        assert out.stdout.split() == ['3', '16', '65536', '1', '0', '1', '0', '0']


def test_binding_takes_the_scene_types_from_the_header_and_leaves_the_other_headers_alone():
    lib = _lib.lib()
    vp, ci, cd = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
    with open(_lib.SCENE_HEADER_PATH) as f:
        text = re.sub(r'/\*.*?\*/', '', f.read(), flags=re.S)
    for name in SCENE_SYMBOLS:
        m = re.search(r'\bint\s+' + name + r'\s*\(([^)]*)\)\s*;', text)
        params = [' '.join(q.split()) for q in m.group(1).split(',')]
        fn = getattr(lib, name)
        assert fn.restype is ci and len(fn.argtypes) == len(params), name
        for at, q in zip(fn.argtypes, params):
            assert at is (vp if '*' in q else {'int': ci, 'double': cd}[q.rsplit(' ', 1)[0]]), (name, q)
    assert tuple(lib.cg_depth_to_xyz.argtypes) == (vp, ci, ci, ci, cd, cd, cd, cd, vp, vp, vp)
    assert tuple(lib.cg_organized_normals.argtypes) == (vp, vp, ci, ci, cd, cd, cd, cd, cd, ci, cd, cd, cd, ci, ci, ci, vp, vp, vp, vp)
    assert tuple(lib.cg_scene_halo_fits.argtypes) == (ci, ci)
    with pytest.raises(ctypes.ArgumentError):
        lib.cg_organized_normals(None, None, 4, 4, 1.0, 1.0, 0.0, 0.0, 0.002, 30.5, 0.0, 0.0, 0.0, 0, 0, 0, None, None, None, None)
    assert lib.cg_organized_normals(None, None, 4, 4, 1.0, 1.0, 0.0, 0.0, 0.002, 30, 0.0, 0.0, 0.0, 0, 0, 0, None, None, None, None) == -1
    assert lib.cg_depth_to_xyz(None, 0, 4, 4, 1.0, 1.0, 0.0, 0.0, None, None, None) == -1
    assert (lib.cg_scene_halo_fits(17, 17), lib.cg_scene_halo_fits(40, 40)) == (1, 0)
    # the other headers' views are unchanged: the main header's 71 functions, and none of the scene ones anywhere else
    assert len(_lib.declared_symbols()) == 71
    for sigs in (_lib.signatures(), _lib.cluster_signatures(), _lib.sparse_signatures(), _lib.pointgroup_signatures()):
        assert not set(SCENE_SYMBOLS) & set(sigs)
    assert sorted(_lib.cluster_signatures()) == ['cg_meanshift_climb', 'cg_meanshift_lds_max_points', 'cg_meanshift_merge']


def test_lib_raises_when_the_library_lacks_a_scene_symbol(monkeypatch):
    real = _lib.scene_signatures()
    monkeypatch.setattr(_lib, '_lib', None)
    monkeypatch.setattr(_lib, 'scene_signatures', lambda: {**real, 'cg_scene_not_built': (ctypes.c_int, ())})
    with pytest.raises(_lib.CatgraspAmdError, match='cg_scene_not_built'):
        _lib.lib()


def test_build_tracks_the_scene_header():
    from catgrasp_amd import build
    import inspect
    assert 'catgrasp_amd_scene.h' in inspect.getsource(build.build)
    assert any(s.endswith('scene.hip') for s in build.sources())


def test_python_refusals_come_before_any_device_work(monkeypatch):
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    depth = np.full((8, 9), 0.5, np.float32)
    bad_depth = [depth.copy() for _ in range(3)]
    bad_depth[0][2, 3], bad_depth[1][0, 0], bad_depth[2][7, 8] = np.nan, np.inf, -np.inf
    for d, fn in itertools.product(bad_depth + [bad_depth[0].astype(np.float64)], (scene.scene_from_depth, scene.depth2xyzmap, pipeline.scene_from_depth)):
        with pytest.raises(ValueError, match='NaN or infinity'):
            fn(d, K)
    for k in (np.eye(4), K[:2], K.reshape(-1), K * [[-1, 1, 1]] * 3, K * [[1, 1, 1], [1, 0, 1], [1, 1, 1]], K * np.nan):
        with pytest.raises(ValueError, match='K '):
            scene.scene_from_depth(depth, k)
        with pytest.raises(ValueError, match='K '):
            scene.depth2xyzmap(depth, k)
        with pytest.raises(ValueError, match='K '):
            scene.estimate_normals_organized(torch.zeros(8, 9, 3), torch.ones(8, 9), k)
    for r in (0.0, -0.002, float('inf'), float('nan')):
        with pytest.raises(ValueError, match='radius'):
            scene.scene_from_depth(depth, K, radius=r)
        with pytest.raises(ValueError, match='radius'):
            scene.estimate_normals_organized(torch.zeros(8, 9, 3), torch.ones(8, 9), K, radius=r)
    for nn in (0, -3, 2.5):
        with pytest.raises(ValueError, match='max_nn'):
            scene.scene_from_depth(depth, K, max_nn=nn)
        with pytest.raises(ValueError, match='max_nn'):
            scene.estimate_normals_organized(torch.zeros(8, 9, 3), torch.ones(8, 9), K, max_nn=nn)
    for kw in (dict(bg_mask=np.zeros((9, 8), bool)), dict(bg_mask=np.zeros((8, 9, 1), bool)), dict(rgb=np.zeros((8, 8, 3), np.uint8))):
        with pytest.raises(ValueError, match='shape'):
            scene.scene_from_depth(depth, K, **kw)
    with pytest.raises(ValueError, match='shape'):
        scene.estimate_normals_organized(torch.zeros(8, 9, 3), torch.ones(9, 8), K)
    with pytest.raises(ValueError, match='route'):
        scene.estimate_normals_organized(torch.zeros(8, 9, 3), torch.ones(8, 9), K, route='lds')
    with pytest.raises(ValueError, match='depth'):
        scene.depth2xyzmap(np.zeros((8, 9, 1), np.float32), K)


def test_without_a_hip_device_the_front_end_raises(monkeypatch):
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)          # on a GPU host too: the refusal, not a CPU fallback
    depth = np.full((8, 9), 0.5, np.float32)
    with pytest.raises(_lib.CatgraspAmdError):
        scene.depth2xyzmap(depth, K)
    with pytest.raises(_lib.CatgraspAmdError):
        scene.depth2xyzmap(depth, K, device='cpu')
    with pytest.raises(_lib.CatgraspAmdError):
        scene.scene_from_depth(depth, K)
    with pytest.raises(_lib.CatgraspAmdError):
        scene.estimate_normals_organized(torch.zeros(8, 9, 3), torch.ones(8, 9), K)
    with pytest.raises(_lib.CatgraspAmdError):
        pipeline.objects_from_depth(depth, K, predictor=None)
    assert pipeline.scene_from_depth is scene.scene_from_depth


def test_scene_kernels_stay_out_of_scratch():
    """Every instantiation of the scene kernels compiles without a private segment and without spilled registers (the selection keeps
    no per-thread list: scripts/kernel_resources.py on the built object; no GPU needed)."""
    import importlib.util
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location('kernel_resources', os.path.join(root, 'scripts', 'kernel_resources.py'))
    kr = importlib.util.module_from_spec(spec); spec.loader.exec_module(kr)
    if not all(os.path.exists(os.path.join(kr.LLVM, t)) for t in ('llvm-objcopy', 'clang-offload-bundler', 'llvm-readelf')) or shutil.which('c++filt') is None:
        pytest.skip('ROCm llvm binutils / c++filt not found')
    obj = os.path.join(root, 'catgrasp_amd', 'csrc', 'scene.o')
    if not os.path.exists(obj):
        pytest.skip('scene.o not built')
    rows = kr.resources(obj)
    names = sorted(r['kernel'].replace('void ', '') for r in rows)
    assert names == ['depth_to_xyz_kernel<double>', 'depth_to_xyz_kernel<float>', 'organized_normals_kernel<false>', 'organized_normals_kernel<true>']
    for r in rows:
        assert r['private_segment_fixed_size'] == 0 and r['vgpr_spill_count'] == 0 and r['sgpr_spill_count'] == 0 and r['agpr_count'] == 0, r
        assert r['group_segment_fixed_size'] == 0                      # the halo is dynamic LDS, sized per launch
