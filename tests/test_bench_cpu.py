"""bench.py --dump-outputs without a GPU: the 64 MB budget and the fixed sample of a large tensor."""
import os

import numpy as np
import torch

import bench


def test_dump_outputs_stays_in_budget_and_samples_the_same_positions(tmp_path):
    g = torch.Generator().manual_seed(3)
    arrays = {'loss': torch.tensor(0.25), 'small': torch.randn(7, 5, generator=g)}
    arrays.update({f'w{i}': torch.randn(600, 500, generator=g) for i in range(60)})       # 72 MB of float32 in all
    bench.dump_outputs(str(tmp_path / 'a'), arrays)
    bench.dump_outputs(str(tmp_path / 'b'), {k: v.double() for k, v in arrays.items()})
    names = sorted(os.listdir(tmp_path / 'a'))
    assert names == sorted(k + '.npy' for k in arrays)
    assert sum(os.path.getsize(tmp_path / 'a' / n) for n in names) <= bench.DUMP_BUDGET_BYTES
    assert np.load(tmp_path / 'a' / 'loss.npy') == np.float32(0.25)
    np.testing.assert_array_equal(np.load(tmp_path / 'a' / 'small.npy'), arrays['small'].numpy())
    w = np.load(tmp_path / 'a' / 'w0.npy')
    assert w.dtype == np.float32 and w.ndim == 1 and 0 < w.size < arrays['w0'].numel()
    assert np.isin(w, arrays['w0'].numpy()).all()
    for n in names:
        np.testing.assert_array_equal(np.load(tmp_path / 'a' / n), np.load(tmp_path / 'b' / n), err_msg=n)
