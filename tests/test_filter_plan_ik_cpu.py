"""CPU tests (no GPU) of the IK stage of the multi-segment filter's C ABI: the entry points are declared and exported, and the ctypes
mirror of cg_iiwa_ik_params has the C struct's layout."""
import ctypes
import os
import shutil
import subprocess

import pytest

from catgrasp_amd import _lib, my_cpp

NEW = ('cg_filter_grasp_pose_multi_ik', 'cg_filter_segments_ee_in_base')


def test_ik_entry_points_are_declared_and_exported():
    syms = _lib.declared_symbols()
    for s in NEW:
        assert s in syms
        assert hasattr(_lib.lib(), s)
    with open(_lib.HEADER_PATH) as f:
        assert '} cg_iiwa_ik_params;' in f.read()


def test_ik_entry_points_reject_bad_arguments():
    """Argument checks come before any device work: a missing IK block or output buffer is an error, an empty table is not."""
    lib = _lib.lib()
    null = ctypes.c_void_p(0)
    one = ctypes.c_void_p(16)
    res = ctypes.c_float(0.0005)
    assert lib.cg_filter_grasp_pose_multi_ik(one, one, 1, one, 1, null, null, null, 0, null, null, 0, res, one, one, one,
                                             null, null, 0, null, null) == -1                      # no cg_iiwa_ik_params
    assert lib.cg_filter_grasp_pose_multi_ik(null, null, -1, one, 1, one, null, null, 0, null, null, 0, res, one, one, one,
                                             null, null, 0, null, null) == -1
    assert lib.cg_filter_segments_ee_in_base(null, null, 0, 1, null, null, null, null, null) == 0     # no segments: nothing to do
    assert lib.cg_filter_segments_ee_in_base(one, one, 1, 1, one, one, null, one, null) == -1         # no ee_out
    seg = (my_cpp._FilterSegmentC * 1)()
    seg[0].first = 5                                                                                  # not a prepared table
    assert lib.cg_filter_segments_ee_in_base(seg, one, 1, 1, one, one, ctypes.c_void_p(32), one, null) == -1


def test_ik_params_mirror_matches_the_c_struct(tmp_path):
    if shutil.which('gcc') is None:
        pytest.skip('gcc not available')
    fields = [name for name, _ in my_cpp._IkParamsC._fields_]
    assert fields == ['cam_in_world', 'ee_in_grasp', 'upper', 'lower']
    src = ('#include "catgrasp_amd.h"\n#include <stddef.h>\n#include <stdio.h>\nint main(void) {\n'
           '  printf("%zu %zu' + ' %zu' * len(fields) + '\\n", sizeof(cg_iiwa_ik_params), _Alignof(cg_iiwa_ik_params)' +
           ''.join(f', offsetof(cg_iiwa_ik_params, {f})' for f in fields) + ');\n  return 0;\n}\n')
    (tmp_path / 'layout.c').write_text(src)
    subprocess.check_call(['gcc', '-std=c11', '-Wall', '-Werror', '-I', os.path.dirname(_lib.HEADER_PATH), 'layout.c', '-o', 'layout'],
                          cwd=tmp_path)
    out = [int(v) for v in subprocess.run([str(tmp_path / 'layout')], capture_output=True, text=True, check=True).stdout.split()]
    C = my_cpp._IkParamsC
    assert out == [ctypes.sizeof(C), ctypes.alignment(C)] + [getattr(C, f).offset for f in fields]
    assert ctypes.sizeof(C) == 240
