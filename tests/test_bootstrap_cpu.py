"""CPU-only: the bootstrap's draw rule on the host oracle alone (conditions on the rule, not measurements of the kernel), the statistics
of evaluate.bootstrap_ci / paired_bootstrap fed oracle sums through their ``sums=`` seam, and mts_bootstrap_sums' argument checks."""
import numpy as np
import pytest

from tests import bootstrap_oracle as oracle

S = 10000


@pytest.mark.parametrize('n', [55, 64, 337])
@pytest.mark.parametrize('seed', [0, 1, 1234])
def test_draw_rule_is_uniform_and_gives_the_normal_half_width(seed, n):
    idx = oracle.draws(seed, n, S)
    assert idx.shape == (S, n) and idx.dtype == np.int64 and idx.min() >= 0 and idx.max() < n
    # every index is drawn S * n times with probability 1 / n: mean S, sigma sqrt(S (1 - 1/n))
    counts = np.bincount(idx.reshape(-1), minlength=n)
    sigma = np.sqrt(S * (1.0 - 1.0 / n))
    worst = np.abs(counts - S).max() / sigma
    print(f'seed {seed} n {n}: largest count deviation {worst:.2f} sigma')
    assert worst <= 5.0
    values = np.random.default_rng(5).random((3, n))
    means = oracle.sums(values, seed, S) / n
    half = (np.percentile(means, 97.5, axis=1) - np.percentile(means, 2.5, axis=1)) / 2
    ratio = half / (1.959964 * values.std(axis=1) / np.sqrt(n))
    print(f'seed {seed} n {n}: half width / normal half width {ratio}')
    assert (ratio >= 0.95).all() and (ratio <= 1.05).all()


def test_oracle_sums_are_sequential_and_paired():
    values = np.array([[1e3, -1e-3, 3.0, 1e-3, -1e3], [1.0, 2.0, 3.0, 4.0, 5.0]])
    idx = oracle.draws(7, 5, 33)
    got = oracle.sums(values, 7, 33)
    for s in range(33):
        for m in range(2):
            acc = 0.0
            for j in range(5):
                acc = acc + values[m, idx[s, j]]
            assert got[m, s] == acc
    assert np.array_equal(oracle.sums(values[1], 7, 33)[0], got[1])                 # the draw does not depend on M: rows stay paired
    assert not np.array_equal(oracle.draws(8, 5, 33), idx)


def test_bootstrap_ci_expressions_through_the_seam():
    from multimodaltopicsegmentation_amd import bootstrap_ci
    rng = np.random.default_rng(3)
    values = rng.random((4, 21)) * np.array([[1e-3], [1.0], [1e3], [-5.0]])
    sums = oracle.sums(values, 11, 500)
    out = bootstrap_ci(values, samples=500, seed=11, sums=sums)
    assert set(out) == {'mean', 'lo', 'hi', 'half_width'} and all(out[k].shape == (4,) for k in out)
    means = sums / 21
    assert np.array_equal(out['mean'], values.mean(axis=1))
    assert np.array_equal(out['lo'], np.percentile(means, 2.5, axis=1)) and np.array_equal(out['hi'], np.percentile(means, 97.5, axis=1))
    assert np.array_equal(out['half_width'], (out['hi'] - out['lo']) / 2)
    assert (out['lo'] < out['mean']).all() and (out['mean'] < out['hi']).all()
    one = bootstrap_ci(values[2], samples=500, seed=11, sums=sums[2])                # [n] in -> arrays of length 1
    assert all(one[k].shape == (1,) and one[k][0] == out[k][2] for k in out)
    with pytest.raises(ValueError):
        bootstrap_ci(values, samples=400, seed=11, sums=sums)                        # sums of another number of resamples
    with pytest.raises(ValueError):
        bootstrap_ci(np.zeros((2, 0)), samples=5, sums=np.zeros((2, 5)))


def test_one_document_has_no_width():
    from multimodaltopicsegmentation_amd import bootstrap_ci
    values = np.array([[0.37], [-2.5]])
    out = bootstrap_ci(values, samples=64, seed=0, sums=oracle.sums(values, 0, 64))
    assert np.array_equal(out['lo'], out['hi']) and np.array_equal(out['lo'], out['mean']) and np.array_equal(out['mean'], values[:, 0])
    assert np.array_equal(out['half_width'], np.zeros(2))


def test_dict_in_gives_dict_out():
    from multimodaltopicsegmentation_amd import bootstrap_ci
    rng = np.random.default_rng(4)
    table = {'Pk': rng.random(17), 'F1': rng.random(17)}
    stacked = np.stack([table['Pk'], table['F1']])
    sums = oracle.sums(stacked, 2, 300)
    out, ref = bootstrap_ci(table, samples=300, seed=2, sums=sums), bootstrap_ci(stacked, samples=300, seed=2, sums=sums)
    for stat in ('mean', 'lo', 'hi', 'half_width'):
        assert list(out[stat]) == ['Pk', 'F1'] and [out[stat]['Pk'], out[stat]['F1']] == ref[stat].tolist()
        assert all(isinstance(v, float) for v in out[stat].values())
    with pytest.raises(ValueError):
        bootstrap_ci({'Pk': np.zeros(3), 'F1': np.zeros(4)}, samples=5, sums=np.zeros((2, 5)))


def test_paired_bootstrap_through_the_seam():
    from multimodaltopicsegmentation_amd import paired_bootstrap
    rng = np.random.default_rng(6)
    a = rng.random(25)
    same = paired_bootstrap(a, a, samples=200, seed=1, sums=oracle.sums(a - a, 1, 200))
    assert same['mean_diff'][0] == 0 and same['p_le_0'][0] == 1 and same['p_ge_0'][0] == 1 and same['lo'][0] == 0 == same['hi'][0]
    b = a - 0.5 - 0.1 * rng.random(25)                                               # a is better by at least 0.5 on every document
    d = a - b
    sums = oracle.sums(d, 1, 200)
    out = paired_bootstrap(a, b, samples=200, seed=1, sums=sums)
    means = sums / 25
    assert out['mean_diff'][0] == d.mean() and out['p_le_0'][0] == 0 and out['p_ge_0'][0] == 1
    assert out['lo'][0] == np.percentile(means[0], 2.5) and out['hi'][0] == np.percentile(means[0], 97.5) and out['lo'][0] >= 0.5
    with pytest.raises(ValueError):
        paired_bootstrap(a, b[:-1], samples=200, seed=1)
    assert 'extension' in paired_bootstrap.__doc__ and 't-test' in paired_bootstrap.__doc__


def test_argument_checks_come_before_any_device_work():
    from multimodaltopicsegmentation_amd import _lib as L
    for n, M, S in ((0, 1, 1), (1, 17, 1), (1, 1, 0), ((1 << 20) + 1, 1, 1), (1, 0, 1), (1, 1, (1 << 22) + 1), (-1, 1, 1)):
        rc = L.lib.mts_bootstrap_sums(None, n, M, S, None, 0, None)
        assert rc == 1, (n, M, S)
        with pytest.raises(ValueError, match='mts_bootstrap_sums'):
            L.check(rc)
    assert L.lib.mts_bootstrap_sums(None, 1, 1, 1, None, 0, None) == 1              # null operands inside the domain
