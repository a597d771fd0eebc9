"""bench.py without a GPU: what --dump-outputs writes (budget, fixed samples, dtypes) and the options a plain run refuses."""
import glob
import os

import numpy as np
import pytest
import torch

_env = dict(os.environ)
import bench  # noqa: E402  (sets HIP environment defaults for its own process: not for this one's GPU tests)
for _k in set(os.environ) - set(_env):
    del os.environ[_k]


class _Opt:
    def __init__(self, n, seed):
        self.param_arena = torch.randn(n, generator=torch.Generator().manual_seed(seed))


def _result():
    g = torch.Generator().manual_seed(7)
    return (torch.tensor(0.25), {'kp': torch.randn(8, generator=g), 'mask': torch.randn(8, 4, generator=g)},
            torch.tensor(1.5, dtype=torch.float64),
            {'preds': {'cam 1': torch.randn(16, 17, 3, generator=g).requires_grad_()}, 'ids': torch.arange(5), 'flag': True})


def test_dump_outputs_budget_samples_and_dtypes(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, 'DUMP_BYTES', 64 * 1024)
    det, dsc = _Opt(100_000, 1), _Opt(3_000, 2)
    a = bench.dump_outputs(str(tmp_path / 'a'), _result(), det, dsc)
    b = bench.dump_outputs(str(tmp_path / 'b'), _result(), det, dsc)
    assert a == b
    files = sorted(os.path.basename(f) for f in glob.glob(str(tmp_path / 'a' / '*.npy')))
    assert files == sorted(n + '.npy' for n in a)
    assert 'info.preds.cam_1.npy' in files and 'params.detector.npy' in files and 'params.discriminator.npy' in files
    data = sum(np.load(str(tmp_path / 'a' / f)).nbytes for f in files)
    assert data <= bench.DUMP_BYTES
    for f in files:
        x, y = np.load(str(tmp_path / 'a' / f)), np.load(str(tmp_path / 'b' / f))
        assert x.dtype in (np.float32, np.float64) and np.array_equal(x, y), f
    assert np.load(str(tmp_path / 'a' / 'total.npy')).dtype == np.float64
    kp = np.load(str(tmp_path / 'a' / 'loss_kp.mask.npy'))                      # small: whole, in its shape
    assert kp.shape == (8, 4) and np.array_equal(kp, _result()[1]['mask'].numpy())
    shape, k = a['params.detector']                                             # large: a sample of its own values
    assert shape == (100_000,) and 0 < k < 100_000
    sample = np.load(str(tmp_path / 'a' / 'params.detector.npy'))
    assert sample.shape == (k,) and np.isin(sample, det.param_arena.numpy()).all()


@pytest.mark.parametrize('extra', [['--shape-report', 'shapes.txt'], ['--ref-n1', '100']])
def test_full_only_options_need_full(monkeypatch, extra):
    monkeypatch.setattr('sys.argv', ['bench.py', '--steps', '1'] + extra)
    with pytest.raises(SystemExit) as e:
        bench.main()
    assert e.value.code == 2
