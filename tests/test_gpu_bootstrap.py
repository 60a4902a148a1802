"""GPU tests of mts_bootstrap_sums (csrc/bootstrap.hip) against the host oracle, bit for bit: the draws are a counter hash and the sums
are ordered float64 additions, so nothing is left to a tolerance.  Both kernel paths: the row staged in LDS (n <= 8192) and read from
global memory beyond that."""
import numpy as np
import pytest
import torch

from tests import bootstrap_oracle as oracle

pytestmark = pytest.mark.gpu
DEV = 'cuda'
# every value of n {1, 2, 55, 64, 65, 337}, M {1, 3, 6, 16} and S {1, 63, 64, 65, 257, 10000} at least once; the tails 65 / 3 / 65 and
# 65 / 16 / 257 together; 8192 is the last n staged in LDS, 8193 and 9000 take the global-memory path
CASES = [(1, 1, 1), (2, 3, 63), (55, 6, 10000), (64, 16, 64), (65, 3, 65), (65, 16, 257), (337, 6, 257), (337, 1, 10000),
         (8192, 2, 65), (8193, 2, 65), (9000, 1, 65)]


def _values(M, n, seed=0):
    """mixed magnitudes 1e-3 .. 1e3, both signs: a sum in another order differs in its last bits"""
    rng = np.random.default_rng(seed)
    return np.where(rng.random((M, n)) < 0.5, -1.0, 1.0) * 10.0 ** rng.uniform(-3, 3, (M, n))


def _kernel(values, S, seed):
    from multimodaltopicsegmentation_amd import ops
    out = ops.bootstrap_sums(torch.from_numpy(values).to(DEV), S, seed)
    assert tuple(out.shape) == (1 if values.ndim == 1 else values.shape[0], S) and out.dtype == torch.float64
    return out.cpu().numpy()


@pytest.mark.parametrize('n,M,S', CASES)
def test_sums_equal_the_oracle_bit_for_bit(n, M, S):
    values = _values(M, n, seed=n + M)
    seed = 1234 + S
    want = oracle.sums(values, seed, S)
    got = _kernel(values, S, seed)
    assert np.array_equal(got, want), np.abs(got - want).max()
    if n > 2 and S > 1:
        assert len(np.unique(got[0])) > 1                                         # resamples differ from one another


def test_seeds_and_repeats():
    values = _values(3, 55, seed=9)
    a, b, c = _kernel(values, 257, 5), _kernel(values, 257, 5), _kernel(values, 257, 6)
    assert np.array_equal(a, b) and not np.array_equal(a, c)
    big = (1 << 63) + 12345                                                        # the whole 64 bits of the seed reach the hash
    assert np.array_equal(_kernel(values, 65, big), oracle.sums(values, big, 65))
    one = _kernel(values[1], 257, 5)                                               # [n] in: the draw does not depend on M
    assert np.array_equal(one[0], a[1])


def test_every_element_is_written_and_the_domain_is_checked():
    from multimodaltopicsegmentation_amd import ops
    values = torch.from_numpy(_values(2, 65)).to(DEV)
    out = torch.full((2, 65), float('nan'), dtype=torch.float64, device=DEV)
    assert ops.bootstrap_sums(values, 65, 3, out=out) is out and not torch.isnan(out).any()
    with pytest.raises(ValueError):
        ops.bootstrap_sums(values, 0, 3)
    with pytest.raises(ValueError):
        ops.bootstrap_sums(torch.zeros(17, 4, dtype=torch.float64, device=DEV), 8, 3)


def test_bootstrap_ci_on_the_device_equals_the_oracle_fed_one():
    from multimodaltopicsegmentation_amd import bootstrap_ci, paired_bootstrap
    rng = np.random.default_rng(2)
    values = rng.random((6, 55))
    got = bootstrap_ci(values, samples=10000, seed=7, device=DEV)
    want = bootstrap_ci(values, samples=10000, seed=7, sums=oracle.sums(values, 7, 10000))
    for k in ('mean', 'lo', 'hi', 'half_width'):
        assert np.array_equal(got[k], want[k]), k
    assert (got['half_width'] > 0).all()
    table = {'Pk': values[0], 'F1': values[2]}
    assert bootstrap_ci(table, samples=257, seed=7) == bootstrap_ci(table, samples=257, seed=7,
                                                                     sums=oracle.sums(np.stack([values[0], values[2]]), 7, 257))
    a, b = values[0], values[1]
    assert all(np.array_equal(x, y) for x, y in zip(paired_bootstrap(a, b, samples=500, seed=1).values(),
                                                    paired_bootstrap(a, b, samples=500, seed=1, sums=oracle.sums(a - b, 1, 500)).values()))
