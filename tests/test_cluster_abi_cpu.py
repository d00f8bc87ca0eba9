"""CPU tests (no GPU) of the clustering step's boundary: include/catgrasp_amd_cluster.h is plain C99 and links from C, the ctypes
binding takes its types from that header, the Python front refuses what it does not build and refuses to run without a HIP device,
and the segment selection orders like the reference."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from catgrasp_amd import _lib, cluster, pipeline, segmentation

INCLUDE = os.path.dirname(_lib.CLUSTER_HEADER_PATH)
CLUSTER_SYMBOLS = ['cg_meanshift_climb', 'cg_meanshift_lds_max_points', 'cg_meanshift_merge']


def test_cluster_header_is_strict_c99_and_links_from_c(tmp_path):
    if shutil.which('gcc') is None:
        pytest.fail('gcc is needed to check the header')
    syms = sorted(_lib.cluster_signatures())
    assert syms == CLUSTER_SYMBOLS
    # both headers in one translation unit, either order of inclusion; every function taken by address; argument errors need no GPU
    src = ('#include "catgrasp_amd_cluster.h"\n#include "catgrasp_amd.h"\n#include "catgrasp_amd_cluster.h"\n#include <stdio.h>\n'
           'typedef void (*fn_t)(void);\nint main(void) {\n  fn_t table[] = {\n' + ''.join(f'    (fn_t)&{s},\n' for s in syms) + '  };\n'
           '  double d[3] = {0, 0, 0}; int i[1]; unsigned char k[1];\n'
           '  int bad = 0;\n'
           '  bad += cg_meanshift_climb(d, 1, 0, d, 1, 0.01, 300, CG_MEANSHIFT_ROUTE_AUTO, d, i, i, (void*)0) != CG_ERR_ARG;   /* n <= 0 */\n'
           '  bad += cg_meanshift_climb((void*)0, 1, 1, d, 1, 0.01, 300, 0, d, i, i, (void*)0) != CG_ERR_ARG;                /* null */\n'
           '  bad += cg_meanshift_climb(d, 1, 1, d, 1, 0.0, 300, 0, d, i, i, (void*)0) != CG_ERR_ARG;                        /* bandwidth */\n'
           '  bad += cg_meanshift_climb(d, 1, 1, d, 1, 1.0 / d[0], 300, 0, d, i, i, (void*)0) != CG_ERR_ARG;                 /* infinite */\n'
           '  bad += cg_meanshift_climb(d, 1, 1, d, 1, 0.01, -1, 0, d, i, i, (void*)0) != CG_ERR_ARG;                        /* max_iter */\n'
           '  bad += cg_meanshift_climb(d, 0, 20000, d, 1, 0.01, 300, CG_MEANSHIFT_ROUTE_LDS, d, i, i, (void*)0) != CG_ERR_ARG; /* no fit */\n'
           '  bad += cg_meanshift_merge(d, 0, 0.01, k, (void*)0) != CG_ERR_ARG;\n'
           '  bad += cg_meanshift_merge(d, 1, -1.0, k, (void*)0) != CG_ERR_ARG;\n'
           '  bad += cg_meanshift_merge(d, 1, 0.01, (unsigned char*)0, (void*)0) != CG_ERR_ARG;\n'
           '  printf("%d %d %d\\n", (int)(sizeof table / sizeof table[0]), cg_meanshift_lds_max_points(0), cg_meanshift_lds_max_points(1));\n'
           '  return bad;\n}\n')
    (tmp_path / 'main.c').write_text(src)
    libdir = os.path.dirname(_lib.LIB_PATH)
    subprocess.check_call(['gcc', '-std=c99', '-Wall', '-Wextra', '-Werror', '-pedantic', '-I', INCLUDE, 'main.c', '-L', libdir, '-lcatgrasp_amd',
                           f'-Wl,-rpath,{libdir}', '-Wl,--allow-shlib-undefined', '-o', 'main'], cwd=tmp_path)
    out = subprocess.run([str(tmp_path / 'main')], capture_output=True, text=True)
    assert out.returncode == 0, (out.returncode, out.stderr)
    assert out.stdout.split() == [str(len(syms)), str(160 * 1024 // 12), str(160 * 1024 // 24)]


def test_binding_takes_the_cluster_types_from_the_header_and_leaves_the_main_header_alone():
    lib = _lib.lib()
    vp, ci, cl, cd = ctypes.c_void_p, ctypes.c_int, ctypes.c_long, ctypes.c_double
    with open(_lib.CLUSTER_HEADER_PATH) as f:
        text = re.sub(r'/\*.*?\*/', '', f.read(), flags=re.S)
    scalars = {'int': ci, 'long': cl, 'double': cd}
    for name in CLUSTER_SYMBOLS:
        m = re.search(r'\bint\s+' + name + r'\s*\(([^)]*)\)\s*;', text)
        params = [' '.join(q.split()) for q in m.group(1).split(',')]
        fn = getattr(lib, name)
        assert fn.restype is ci and len(fn.argtypes) == len(params), name
        for at, q in zip(fn.argtypes, params):
            assert at is (vp if '*' in q else scalars[q.rsplit(' ', 1)[0]]), (name, q)
    assert tuple(lib.cg_meanshift_climb.argtypes) == (vp, ci, ci, vp, cl, cd, ci, ci, vp, vp, vp, vp)
    assert tuple(lib.cg_meanshift_merge.argtypes) == (vp, ci, cd, vp, vp)
    with pytest.raises(ctypes.ArgumentError):
        lib.cg_meanshift_merge(None, 1.5, 0.01, None, None)                      # a float for the int count never reaches C
    assert lib.cg_meanshift_merge(None, 1, 0.01, None, None) == -1
    # the main header's view is unchanged: its 71 functions, none of the cluster ones
    assert len(_lib.declared_symbols()) == 71 and not set(CLUSTER_SYMBOLS) & set(_lib.declared_symbols())
    assert set(_lib.signatures()) == set(_lib.declared_symbols())


def test_lib_raises_when_the_library_lacks_a_cluster_symbol(monkeypatch):
    real = _lib.cluster_signatures()
    monkeypatch.setattr(_lib, '_lib', None)
    monkeypatch.setattr(_lib, 'cluster_signatures', lambda: {**real, 'cg_meanshift_not_built': (ctypes.c_int, ())})
    with pytest.raises(_lib.CatgraspAmdError, match='cg_meanshift_not_built'):
        _lib.lib()


def test_constructor_refusals():
    with pytest.raises(NotImplementedError):
        cluster.MeanShift(bandwidth=None)
    with pytest.raises(NotImplementedError):
        cluster.MeanShift()
    with pytest.raises(NotImplementedError):
        cluster.MeanShift(bandwidth=0.007, bin_seeding=True)
    for bw in (0.0, -0.007, float('inf'), float('nan')):
        with pytest.raises(ValueError):
            cluster.MeanShift(bandwidth=bw)
    with pytest.raises(ValueError):
        cluster.MeanShift(bandwidth=0.007, max_iter=-1)
    ms = cluster.MeanShift(bandwidth=0.007, cluster_all=True, n_jobs=-1, seeds=None)       # the reference's call
    assert (ms.bandwidth, ms.cluster_all, ms.seeds, ms.max_iter) == (0.007, True, None, 300)
    with pytest.raises(NotImplementedError):
        segmentation.instances_from_offsets(np.zeros((4, 3)), np.zeros((4, 3), np.float32), np.zeros((4, 3), np.float32), class_name='bolt')


def test_fit_without_a_hip_device_raises(monkeypatch):
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)          # on a GPU host too: the refusal, not a CPU fallback
    X = np.random.default_rng(0).normal(0, 0.001, (50, 3)).astype(np.float32)
    with pytest.raises(_lib.CatgraspAmdError):
        cluster.MeanShift(bandwidth=0.007).fit(X)
    with pytest.raises(_lib.CatgraspAmdError):
        cluster.climb(torch.from_numpy(X), torch.from_numpy(X).double(), 0.007)
    with pytest.raises(_lib.CatgraspAmdError):
        segmentation.instances_from_offsets(X, X, np.zeros_like(X), class_name='nut')


def _boxes(spec):
    """spec: [(label, n points, extent in mm)] -> cloud and labels; every box gets its two extreme corners."""
    rng = np.random.default_rng(7)
    xyz, lab = [], []
    for k, (label, n, ext) in enumerate(spec):
        p = rng.uniform(0, 1, (n, 3))
        p[0], p[1] = 0.0, 1.0
        xyz.append(p * np.asarray(ext) * 0.001 + [0.1 * k, 0, 0.5])
        lab.append(np.full(n, label))
    perm = rng.permutation(sum(n for _, n, _ in spec))
    return np.concatenate(xyz)[perm], np.concatenate(lab)[perm].astype(np.int64)


def test_select_segments_order_tie_rule_and_rejections():
    spec = [(0, 600, (20, 20, 2)),        # density 600 / 800 = 0.75
            (1, 800, (20, 20, 4)),
            (2, 600, (10, 20, 4)),        # ties with 0: the larger label goes first
            (3, 499, (10, 10, 2)),        # one point short
            (4, 500, (10, 10, 2)),        # exactly min_points: stays
            (5, 700, (50, 50, 50)),       # 700 / 125000 = 0.0056 < 0.01: too sparse
            (7, 1000, (50, 50, 39))]      # 1000 / 97500 = 0.0103: just dense enough (and ids need not be consecutive)
    xyz, lab = _boxes(spec)
    cleaned, order = segmentation.select_segments(xyz, lab)
    assert order.tolist() == [7, 1, 2, 0, 4] and order.dtype == np.int64
    want = np.where(np.isin(lab, [3, 5]), -1, lab)
    assert np.array_equal(cleaned, want) and cleaned.dtype == np.int64
    # tensors in, the same out; a -1 that is already there stays out of the order
    lab2 = np.where(lab == 1, -1, lab)
    cleaned2, order2 = segmentation.select_segments(torch.from_numpy(xyz), torch.from_numpy(lab2))
    assert order2.tolist() == [7, 2, 0, 4] and np.array_equal(cleaned2, np.where(np.isin(lab2, [3, 5]), -1, lab2))
    # nothing survives
    cleaned3, order3 = segmentation.select_segments(xyz, lab, min_points=5000)
    assert order3.tolist() == [] and (cleaned3 == -1).all()

    nrm = np.random.default_rng(1).normal(size=xyz.shape)
    obs = pipeline.objects_from_segmentation(xyz, nrm, cleaned, order)
    assert [len(o['ob_pts']) for o in obs] == [1000, 800, 600, 600, 500]
    for o, seg in zip(obs, order):
        assert np.array_equal(o['ob_pts'], xyz[lab == seg]) and np.array_equal(o['ob_normals'], nrm[lab == seg])
