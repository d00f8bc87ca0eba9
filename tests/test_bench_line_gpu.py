"""GPU: the plain bench line (no --full) and --dump-outputs.  A plain run carries the contract's fields and none of the --full blocks;
the dumped records are the ones `records_sha256` hashes, and two runs with the same arguments dump identical records."""
import hashlib
import os
import sys

import numpy as np
import pytest

from test_bench_multirank_gpu import _run

pytestmark = pytest.mark.gpu
FULL_ONLY = {'secondary', 'api', 'pp_encoder', 'projected_scaling', 'rccl_selftest', 'roofline_filter', 'configs', 'cpu_baseline'}


def test_plain_line_and_dumped_records(cuda_device, tmp_path):
    cmd = [sys.executable, 'bench.py', '--gpus', '1', '--steps', '2', '--warmup', '1', '--candidates', '6000']
    env = dict(os.environ)
    lines = [_run(cmd + ['--dump-outputs', str(tmp_path / tag)], env) for tag in ('a', 'b')]
    for line in lines:
        for key in ('metric', 'value', 'unit', 'n_gpus', 'steps', 'warmup', 'ms_per_step', 'higher_is_better', 'scaling', 'vs_baseline', 'dtype',
                    'data', 'config', 'roofline', 'per_rank_ms', 'records_sha256'):
            assert key in line, key
        assert not FULL_ONLY & set(line), FULL_ONLY & set(line)
        assert line['steps'] == 2 and line['warmup'] == 1 and line['config']['candidates_total'] == 6000
        assert abs(line['value'] * line['ms_per_step'] / 1e3 - 6000) <= 6000 * 1e-3
    recs = [np.load(tmp_path / tag / 'records.npy') for tag in ('a', 'b')]
    for line, rec in zip(lines, recs):
        assert rec.dtype == np.float32 and rec.shape == (6000, 2)
        assert hashlib.sha256(rec.tobytes()).hexdigest() == line['records_sha256']
    assert np.array_equal(recs[0], recs[1])
    assert not (tmp_path / 'a' / 'records_rows.npy').exists()
