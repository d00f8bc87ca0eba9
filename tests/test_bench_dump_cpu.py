"""CPU tests (no GPU) of bench.py --dump-outputs: the records are written as they were returned, float32 in global candidate order; a
batch above the size limit is written as a fixed, seeded, ascending sample of rows together with their candidate indices."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
import bench  # noqa: E402


def _records(n):
    return torch.stack([torch.linspace(0, 1, n), torch.arange(n) % 5.0], dim=1).contiguous()


def test_dump_writes_every_record(tmp_path):
    rec = _records(1000)
    bench.dump_outputs(str(tmp_path / 'out'), rec)
    got = np.load(tmp_path / 'out' / 'records.npy')
    assert got.dtype == np.float32 and np.array_equal(got, rec.numpy())
    assert sorted(os.listdir(tmp_path / 'out')) == ['records.npy']


def test_dump_above_the_limit_writes_a_fixed_sample(tmp_path):
    rec = _records(1000)
    limit = 1600                                                    # 100 rows of 8 B records + 8 B indices
    bench.dump_outputs(str(tmp_path / 'a'), rec, limit_bytes=limit)
    bench.dump_outputs(str(tmp_path / 'b'), rec, limit_bytes=limit)
    rows = np.load(tmp_path / 'a' / 'records_rows.npy')
    got = np.load(tmp_path / 'a' / 'records.npy')
    assert rows.dtype == np.float64 and len(rows) == 100 and np.all(np.diff(rows) > 0)
    assert got.dtype == np.float32 and np.array_equal(got, rec.numpy()[rows.astype(np.int64)])
    assert got.nbytes + rows.nbytes <= limit
    assert np.array_equal(rows, np.load(tmp_path / 'b' / 'records_rows.npy')) and np.array_equal(got, np.load(tmp_path / 'b' / 'records.npy'))
