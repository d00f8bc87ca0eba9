"""CPU tests (no GPU) of the boundary of the NUNOCS loss: include/catgrasp_amd_loss.h is plain C99, alone and after the other ten
headers in either order, and links from C; every argument error and every limit comes back without a GPU; the workspace size is a
function of the shapes; the ctypes binding takes its types from that header and lib() requires its symbols; the build tracks it; the
Python wrapper refuses CPU tensors and strides it would have to copy before any device work."""
import ctypes
import inspect
import os
import re
import shutil
import subprocess

import pytest
import torch

from catgrasp_amd import _lib, loss

INCLUDE = os.path.dirname(_lib.LOSS_HEADER_PATH)
LOSS_SYMBOLS = ['cg_nocs_symce_backward', 'cg_nocs_symce_forward', 'cg_nocs_symce_workspace_floats']
HEADERS = ['catgrasp_amd.h', 'catgrasp_amd_cluster.h', 'catgrasp_amd_sparse.h', 'catgrasp_amd_pointgroup.h', 'catgrasp_amd_scene.h',
           'catgrasp_amd_neighbors.h', 'catgrasp_amd_kdtree.h', 'catgrasp_amd_sparse_grad.h', 'catgrasp_amd_bn.h', 'catgrasp_amd_screen.h']
GCC = ['gcc', '-std=c99', '-Wall', '-Wextra', '-Werror', '-pedantic', '-I', INCLUDE]


def test_loss_header_is_strict_c99_alone_and_after_the_other_ten_and_links_from_c(tmp_path):
    if shutil.which('gcc') is None:
        pytest.fail('gcc is needed to check the header')
    assert sorted(_lib.loss_signatures()) == LOSS_SYMBOLS
    assert sorted(os.listdir(INCLUDE)) == sorted(HEADERS + ['catgrasp_amd_loss.h'])               # the eleventh header
    fwd = 'cg_nocs_symce_forward({pred}, {layout}, {target}, {tfs}, {B}, {N}, {bins}, {S}, {ws}, {loss}, {ids}, {L}, {lse}, (void*)0)'
    bwd = 'cg_nocs_symce_backward({pred}, {layout}, {target}, {tfs}, {lse}, {ids}, {g}, {B}, {N}, {bins}, {S}, {grad}, (void*)0)'
    good = dict(pred='f', layout='CG_NOCS_POINT_MAJOR', target='f', tfs='f', B='2L', N='5L', bins='100', S='12', ws='f', loss='f', ids='i', L='f',
                lse='f', g='f', grad='f')
    # the host arrays stand in for device memory: nothing may be launched, so nothing reads them
    null, inull = '(float*)0', '(int*)0'
    shapes = [(dict(B='0L'), 'CG_ERR_ARG'), (dict(N='0L'), 'CG_ERR_ARG'), (dict(N='16777217L'), 'CG_ERR_ARG'), (dict(bins='0'), 'CG_ERR_ARG'),
              (dict(S='0'), 'CG_ERR_ARG'), (dict(bins='129'), 'CG_ERR_UNSUPPORTED'), (dict(S='129'), 'CG_ERR_UNSUPPORTED'),
              (dict(B='65536L'), 'CG_ERR_UNSUPPORTED'), (dict(layout='2'), 'CG_ERR_ARG'), (dict(layout='-1'), 'CG_ERR_ARG'),
              (dict(bins='129', N='0L'), 'CG_ERR_ARG')]                                           # the counts are judged before the caps
    cases = [(call, b, want) for call in (fwd, bwd) for b, want in shapes]
    cases += [(fwd, b, 'CG_ERR_ARG') for b in (dict(pred=null), dict(target=null), dict(tfs=null), dict(ws=null), dict(loss=null), dict(ids=inull),
                                              dict(L=null))]
    cases += [(bwd, b, 'CG_ERR_ARG') for b in (dict(pred=null), dict(target=null), dict(tfs=null), dict(lse=null), dict(ids=inull), dict(g=null),
                                              dict(grad=null))]
    body = ''.join(f'  bad += {call.format(**{**good, **b})} != {want};   /* {b} */\n' for call, b, want in cases)
    for B, N, bins, S, want in ((1, 1, 4, 1, 1), (3, 64, 100, 12, 36), (3, 65, 100, 12, 72), (34, 8192, 100, 72, 34 * 128 * 72),
                                (65535, 16777216, 128, 128, 65535 * 262144 * 128)):
        body += f'  bad += cg_nocs_symce_workspace_floats({B}L, {N}L, {bins}, {S}) != {want}L;\n'
    body += ('  bad += cg_nocs_symce_workspace_floats(2L, 5L, 129, 12) != CG_ERR_UNSUPPORTED;\n'
             '  bad += cg_nocs_symce_workspace_floats(2L, 5L, 100, 129) != CG_ERR_UNSUPPORTED;\n'
             '  bad += cg_nocs_symce_workspace_floats(0L, 5L, 100, 12) != CG_ERR_ARG;\n'
             '  bad += cg_nocs_symce_workspace_floats(2L, 16777217L, 100, 12) != CG_ERR_ARG;\n')
    for k, order in enumerate((HEADERS, HEADERS[::-1])):
        src = (''.join(f'#include "{h}"\n' for h in order) + '#include "catgrasp_amd_loss.h"\n#include "catgrasp_amd_loss.h"\n#include <stdio.h>\n'
               'typedef void (*fn_t)(void);\nint main(void) {\n  fn_t table[] = {\n' + ''.join(f'    (fn_t)&{s},\n' for s in LOSS_SYMBOLS)
               + '  };\n  float f[4];\n  int i[4];\n  int bad = 0;\n  f[0] = 0.f;\n  i[0] = 0;\n' + body
               + '  printf("%d %d %d %d %d %d\\n", (int)(sizeof table / sizeof table[0]), CG_NOCS_SEG, CG_NOCS_MAX_BINS, CG_NOCS_MAX_SYM,\n'
               '         CG_NOCS_CHANNEL_MAJOR, CG_NOCS_POINT_MAJOR);\n  return bad;\n}\n')
        (tmp_path / f'main{k}.c').write_text(src)
        libdir = os.path.dirname(_lib.LIB_PATH)
        subprocess.check_call(GCC + [f'main{k}.c', '-L', libdir, '-lcatgrasp_amd', f'-Wl,-rpath,{libdir}', '-Wl,--allow-shlib-undefined', '-o', f'main{k}'],
                              cwd=tmp_path)
        out = subprocess.run([str(tmp_path / f'main{k}')], capture_output=True, text=True)
        assert out.returncode == 0, (out.returncode, out.stdout, out.stderr)
        assert out.stdout.split() == ['3', '64', '128', '128', '0', '1']
    (tmp_path / 'alone.c').write_text('#include "catgrasp_amd_loss.h"\nint main(void) { return CG_OK; }\n')
    subprocess.check_call(GCC + ['-fsyntax-only', 'alone.c'], cwd=tmp_path)


def test_binding_takes_the_loss_types_from_the_header_and_leaves_the_other_headers_alone():
    lib = _lib.lib()
    vp, ci, cl = ctypes.c_void_p, ctypes.c_int, ctypes.c_long
    assert tuple(lib.cg_nocs_symce_workspace_floats.argtypes) == (cl, cl, ci, ci) and lib.cg_nocs_symce_workspace_floats.restype is cl
    assert tuple(lib.cg_nocs_symce_forward.argtypes) == (vp, ci, vp, vp, cl, cl, ci, ci) + (vp,) * 6 and lib.cg_nocs_symce_forward.restype is ci
    assert tuple(lib.cg_nocs_symce_backward.argtypes) == (vp, ci) + (vp,) * 5 + (cl, cl, ci, ci, vp, vp) and lib.cg_nocs_symce_backward.restype is ci
    for name in LOSS_SYMBOLS:
        assert hasattr(lib, name)                                                            # exported and bound
    with pytest.raises(ctypes.ArgumentError):
        lib.cg_nocs_symce_workspace_floats(2, 5, 100.0, 12)                                  # a float for bins never reaches C
    assert [lib.cg_nocs_symce_workspace_floats(3, n, 100, 12) for n in (1, 63, 64, 65, 130)] == [36, 36, 36, 72, 108]
    assert lib.cg_nocs_symce_workspace_floats(34, 8192, 100, 72) == 34 * 128 * 72
    assert lib.cg_nocs_symce_workspace_floats(2 ** 16 - 1, 2 ** 24, 128, 128) == (2 ** 16 - 1) * 2 ** 18 * 128   # a long, past 2^31
    assert [lib.cg_nocs_symce_workspace_floats(*a) for a in ((2, 5, 129, 12), (2, 5, 100, 129), (0, 5, 100, 12), (2, 0, 100, 12))] == [-2, -2, -1, -1]
    assert lib.cg_nocs_symce_forward(None, 0, None, None, 2, 5, 100, 12, None, None, None, None, None, None) == -1
    assert lib.cg_nocs_symce_forward(None, 0, None, None, 2, 5, 129, 12, None, None, None, None, None, None) == -2
    assert lib.cg_nocs_symce_backward(None, 1, None, None, None, None, None, 2, 5, 100, 12, None, None) == -1
    assert lib.cg_nocs_symce_backward(None, 1, None, None, None, None, None, 2, 5, 100, 129, None, None) == -2
    for sigs in (_lib.signatures(), _lib.cluster_signatures(), _lib.sparse_signatures(), _lib.pointgroup_signatures(), _lib.scene_signatures(),
                 _lib.neighbors_signatures(), _lib.kdtree_signatures(), _lib.sparse_grad_signatures(), _lib.bn_signatures(), _lib.screen_signatures()):
        assert not set(LOSS_SYMBOLS) & set(sigs)
    assert len(_lib.signatures()) == 71                                                      # the main header stays as it was


def test_lib_raises_when_the_library_lacks_a_loss_symbol(monkeypatch):
    real = _lib.loss_signatures()
    monkeypatch.setattr(_lib, '_lib', None)
    monkeypatch.setattr(_lib, 'loss_signatures', lambda: {**real, 'cg_nocs_not_built': (ctypes.c_int, ())})
    with pytest.raises(_lib.CatgraspAmdError, match='cg_nocs_not_built'):
        _lib.lib()


def test_build_tracks_the_loss_header_and_the_kernels_keep_to_the_stated_arithmetic():
    from catgrasp_amd import build
    assert 'catgrasp_amd_loss.h' in inspect.getsource(build.build)
    src = [s for s in build.sources() if s.endswith('nocs_loss.hip')]
    assert len(src) == 1
    with open(src[0]) as f:
        text = f.read()
    assert 'catgrasp_amd_loss.h' in text and 'fmaf(' in text and 'atomic' not in text.lower() and 'asm' not in text
    assert '-ffp-contract=off' in build.FLAGS and os.path.basename(src[0]) not in build.EXTRA_FLAGS
    with open(_lib.LOSS_HEADER_PATH) as f:
        header = f.read()
    for line in ('loss.py:16-45', 'loss.py:29-45', 'trainer_nunocs.py:52,81', 'fmaf(T[a][2], c_2, fmaf(T[a][1], c_1, fmaf(T[a][0], c_0, T[a][3]))) + 0.5f',
                 '(float)bins', 'CG_NOCS_SEG'):
        assert line in header, line
    assert len(re.findall(r'\bcg_nocs_symce_\w+\s*\(', re.sub(r'/\*.*?\*/', '', header, flags=re.S))) == 3


def test_wrapper_refuses_cpu_tensors_and_strides_it_would_have_to_copy():
    B, N, bins = 2, 6, 4
    pred, target = torch.zeros(B, N, 3 * bins), torch.rand(B, N, 3)
    crit = loss.NocsMinSymmetryCELoss({'nocs_class_name': 'nut', 'ce_loss_bins': bins})
    assert crit.n_sym == 12 and crit.bins == bins and crit.symmetry_tfs().shape == (12, 4, 4) and crit.symmetry_tfs().dtype == torch.float32
    assert loss.NocsMinSymmetryCELoss({'nocs_class_name': 'screw', 'ce_loss_bins': 100}).n_sym == 72
    with pytest.raises(_lib.CatgraspAmdError, match='no CPU fallback'):
        crit(pred, target)
    with pytest.raises(_lib.CatgraspAmdError, match='no CPU fallback'):
        loss.nocs_symce(pred, target, crit.symmetry_tfs(), bins)
    assert loss.layout_of(pred) == loss.POINT_MAJOR
    assert loss.layout_of(torch.zeros(B, 3 * bins, N).permute(0, 2, 1)) == loss.CHANNEL_MAJOR
    for bad in (torch.zeros(N, B, 3 * bins).permute(1, 0, 2), torch.zeros(B, N, 6 * bins)[:, :, ::2], torch.zeros(3 * bins, N, B).permute(2, 1, 0),
                torch.zeros(B, N * 3 * bins)):
        with pytest.raises(ValueError):
            loss.layout_of(bad)
    with pytest.raises(RuntimeError, match='not found'):
        loss.NocsMinSymmetryCELoss({'nocs_class_name': 'bolt', 'ce_loss_bins': bins})
