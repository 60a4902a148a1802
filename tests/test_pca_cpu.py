"""The host half of the PCA projection, no GPU: the NumPy oracle against sklearn (where installed), pca_from_moments against the oracle,
the cancellation of the centre, the reducer's state round trip, project_folds' train-only rule, every refusal of the Python layer and the
return codes of the three C entry points on arguments they must refuse before any device work."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import pca_oracle as O

K = O.PLANTED_K


def labels_of(rows, seed=0):
    """0 / 1 labels for documents of the listed lengths: boundary share 0.2, the last label 0 (the loader's rule)"""
    g = np.random.default_rng([29, seed])
    out = []
    for n in rows:
        y = (g.random(n) < 0.2).astype(np.float32)
        y[-1] = 0.0
        out.append(y.tolist())
    return out


def corpus_of(matrix, rows, device, wire='fp32', second=None, seed=0, segments=None, **kw):
    """a ResidentCorpus whose documents are consecutive row blocks of ``matrix`` (fp32 [sum(rows), D]; ``second`` likewise)"""
    from multimodaltopicsegmentation_amd import AudioPortionDataset, ResidentCorpus
    cut = np.concatenate([[0], np.cumsum(rows)])
    assert cut[-1] == matrix.shape[0]

    def lines(m):
        return [(torch.from_numpy(np.array(m[a:b])), y, f'doc{k}.wav') for k, (a, b, y) in enumerate(zip(cut[:-1], cut[1:], labels_of(rows, seed)))]
    ds = AudioPortionDataset(lines(matrix), {'O': 0, 'B': 1}, CRF=False, truncate=False, second_input=None if second is None else lines(second), **kw)
    return ResidentCorpus(ds, device, wire_dtype=wire, segments=segments)


def _same_reducer(r, f, lam1):
    """the reducer's eigenvalues equal the oracle fit's to 1e-12 lambda_1 and its components to 1e-9, after the sign rule has been
    verified on both sides (so no sign is chosen here)"""
    assert O.sign_rule_holds(r.components_) and O.sign_rule_holds(f['components'])
    assert np.abs(r.explained_variance_ - f['explained_variance']).max() <= 1e-12 * lam1
    assert np.abs(r.components_ - f['components']).max() <= 1e-9
    assert np.abs(r.mean_ - f['mean']).max() <= 1e-12
    assert np.abs(r.explained_variance_ratio_ - f['explained_variance_ratio']).max() <= 1e-12
    assert np.abs(r.singular_values_ - f['singular_values']).max() <= 1e-12 * np.sqrt(lam1 * (r.n_samples_ - 1))


def test_the_planted_spectrum_is_well_separated():
    lam = O.fit(O.planted_matrix(), K)['spectrum']
    gaps = lam[:K] - lam[1:K + 1]
    print('eigenvalues', lam[:K + 1], 'smallest gap', gaps.min(), 'smallest relative gap', (gaps / lam[:K]).min())
    assert 30 < lam[0] < 42 and gaps.min() > 0.1 and (gaps / lam[:K]).min() > 0.1
    x = O.planted_matrix()
    assert np.abs(x).max() <= 8 and np.array_equal(x, np.rint(x))


def test_the_oracle_agrees_with_sklearn():
    pytest.importorskip('sklearn')
    from sklearn.decomposition import PCA
    x = O.planted_matrix().astype(np.float64)
    p = PCA(n_components=K, svd_solver='full').fit(x)
    f = O.fit(x, K)
    assert O.sign_rule_holds(p.components_) and O.sign_rule_holds(f['components'])
    assert np.abs(p.components_ - f['components']).max() <= 1e-9
    assert np.abs(p.explained_variance_ - f['explained_variance']).max() <= 1e-9
    assert np.abs(p.explained_variance_ratio_ - f['explained_variance_ratio']).max() <= 1e-9
    assert np.abs(p.singular_values_ - f['singular_values']).max() <= 1e-9 * f['singular_values'][0]
    assert np.abs(p.mean_ - f['mean']).max() <= 1e-12
    assert np.abs(p.transform(x) - (x - f['mean'][None, :]) @ f['components'].T).max() <= 1e-9


def test_pca_from_moments_equals_the_oracle_fit_and_the_centre_cancels():
    from multimodaltopicsegmentation_amd import PcaReducer, pca_from_moments
    x = O.planted_matrix()
    n, D = x.shape
    f = O.fit(x, K)
    lam1 = f['spectrum'][0]
    s = O.colsum(x)
    near = (s / n).astype(np.float32)                               # the product's choice: fp32 of the mean
    far = O.integer_center(D) + 3.0                                 # an arbitrary other centre
    for c in (near, far, np.zeros(D, dtype=np.float32)):
        xc = x.astype(np.float64) - c.astype(np.float64)[None, :]   # exact moments about c
        r = pca_from_moments(n, s, c, xc.T @ xc, K)
        assert isinstance(r, PcaReducer)
        assert (r.n_components_, r.n_samples_, r.n_features_in_) == (K, n, D)
        assert r.components_.shape == (K, D) and r.components_.dtype == np.float64
        _same_reducer(r, f, lam1)
        assert np.abs((r.components_ ** 2).sum(axis=1) - 1).max() <= 1e-12
    # the largest admissible number of components, and one component
    for k in (1, D):
        r = pca_from_moments(n, s, near, O.gram(x, near), k)
        assert r.components_.shape == (k, D) and np.all(np.diff(r.explained_variance_) <= 0)


def test_sign_rule_takes_the_lowest_index_on_ties():
    from multimodaltopicsegmentation_amd import pca_from_moments
    # two columns, perfectly anticorrelated: the component is (+-1, -+1) / sqrt(2), a tie in magnitude; index 0 is made positive
    x = np.array([[1.0, -1.0], [-1.0, 1.0], [2.0, -2.0], [-2.0, 2.0]])
    r = pca_from_moments(4, x.sum(0), np.zeros(2), x.T @ x, 1)
    assert r.components_[0, 0] > 0 > r.components_[0, 1]
    assert abs(r.explained_variance_[0] - 20.0 / 3.0) < 1e-12 and abs(r.explained_variance_ratio_[0] - 1.0) < 1e-12


def test_state_dict_round_trip():
    from multimodaltopicsegmentation_amd import PcaReducer, pca_from_moments
    x = O.planted_matrix()
    c = np.zeros(x.shape[1], dtype=np.float32)
    r = pca_from_moments(x.shape[0], O.colsum(x), c, O.gram(x, c), K)
    d = r.state_dict()
    assert all(isinstance(v, (np.ndarray, int)) for v in d.values())
    back = PcaReducer.from_state_dict(d)
    for key in ('mean_', 'components_', 'explained_variance_', 'explained_variance_ratio_', 'singular_values_'):
        assert np.array_equal(getattr(back, key), getattr(r, key)), key
        assert d[key] is not getattr(r, key)
    for key in ('n_components_', 'n_samples_', 'n_features_in_'):
        assert getattr(back, key) == getattr(r, key) == d[key]
    d['n_features_in_'] += 1
    with pytest.raises(ValueError):
        PcaReducer.from_state_dict(d)


def test_project_folds_fits_on_train_only(monkeypatch):
    """project_folds on CPU-device corpora.  The device steps of fit_pca and projected are stood in for by the oracle's moments (a CPU
    corpus refuses them: see the refusals below), so what is tested is project_folds' own rule: the fold's reducer comes from ``train``
    alone -- ``val`` and ``test`` hold rows that would change it -- and is applied to all three; ``val`` may be None."""
    from multimodaltopicsegmentation_amd import ResidentCorpus, pca_from_moments, project_folds
    x = O.planted_matrix()
    shifted = (x[:300] * 0 + 7.0).astype(np.float32)                 # rows that would move the mean and the leading component
    shifted[:, :3] = -8.0
    train = corpus_of(x[:1500], [700, 800], 'cpu')
    val = corpus_of(shifted, [300], 'cpu')
    test = corpus_of(np.concatenate([x[1500:], shifted[:10]]), [736, 10], 'cpu')
    fitted, applied = [], []

    def fit_pca(self, n_components=167, field='embeddings', return_moments=False):
        m = self.corpus.numpy()
        c = np.zeros(m.shape[1], dtype=np.float32)
        fitted.append(self)
        return pca_from_moments(m.shape[0], O.colsum(m), c, O.gram(m, c), n_components)

    def projected(self, reducer, reducer2=None):
        applied.append((self, reducer))
        return ('projected', self, reducer)
    monkeypatch.setattr(ResidentCorpus, 'fit_pca', fit_pca)
    monkeypatch.setattr(ResidentCorpus, 'projected', projected)
    folds, reducers = project_folds([(train, val, test), (train, None, test)], n_components=K)
    assert fitted == [train, train] and len(reducers) == 2
    want = O.fit(x[:1500], K)
    with_val = O.fit(np.concatenate([x[:1500], shifted]), K)
    assert np.abs(with_val['components'] - want['components']).max() > 1e-2          # the val rows WOULD change the answer
    for r in reducers:
        _same_reducer(r, want, want['spectrum'][0])
    assert [a for a, _ in applied] == [train, val, test, train, test]
    assert all(r is reducers[0] for _, r in applied[:3]) and all(r is reducers[1] for _, r in applied[3:])
    assert folds[0] == (('projected', train, reducers[0]), ('projected', val, reducers[0]), ('projected', test, reducers[0]))
    assert folds[1][1] is None and folds[1][0][1] is train and folds[1][2][1] is test


def test_refusals_of_the_python_layer():
    from multimodaltopicsegmentation_amd import pca_from_moments
    x = O.planted_matrix()
    D = x.shape[1]
    one = corpus_of(x[:300], [100, 200], 'cpu')
    two = corpus_of(x[:300], [100, 200], 'cpu', second=np.ascontiguousarray(x[:300, :7]))
    single = corpus_of(x[:1], [1], 'cpu')
    for bad in (0.5, 9.0, 'mle', None, True):
        with pytest.raises(ValueError):
            one.fit_pca(bad)
    for bad in (0, -1, D + 1, 301):
        with pytest.raises(ValueError):
            one.fit_pca(bad)
    with pytest.raises(ValueError):
        two.fit_pca(8, field='embeddings2')                          # min(N, D) of the second input is 7
    with pytest.raises(ValueError):
        single.fit_pca(1)                                            # N < 2
    with pytest.raises(ValueError):
        one.fit_pca(K, field='embeddings2')                          # no second input
    with pytest.raises(ValueError):
        one.fit_pca(K, field='targets')
    for corpus, kw in ((one, {}), (two, {'field': 'embeddings2', 'n_components': 7}), (one, {'n_components': np.int64(5)})):
        with pytest.raises(RuntimeError):
            corpus.fit_pca(**{'n_components': K, **kw})              # valid arguments: a CPU-device corpus has no fallback
    c = np.zeros(D, dtype=np.float32)
    r = pca_from_moments(300, O.colsum(x[:300]), c, O.gram(x[:300], c), K)
    r7 = pca_from_moments(300, O.colsum(x[:300, :7]), c[:7], O.gram(x[:300, :7], c[:7]), 3)
    with pytest.raises(RuntimeError):
        r.transform(torch.zeros(4, D))                               # a host tensor
    with pytest.raises(RuntimeError):
        one.projected(r)
    with pytest.raises(ValueError):
        one.projected(r7)                                            # fitted on another width
    with pytest.raises(ValueError):
        one.projected(r, r7)                                         # no second input
    with pytest.raises(ValueError):
        two.projected(r, r)                                          # reducer2 of another width
    with pytest.raises(ValueError):
        pca_from_moments(300, O.colsum(x[:300]), c, O.gram(x[:300], c)[:-1], K)
    with pytest.raises(ValueError):
        pca_from_moments(300, O.colsum(x[:300]), c, O.gram(x[:300], c), 2.0)


def test_load_time_projection_is_still_refused_and_points_to_the_corpus():
    from multimodaltopicsegmentation_amd import AudioPortionDataset, load_dataset_from_precomputed
    with pytest.raises(NotImplementedError, match='fit_pca'):
        AudioPortionDataset([], {'O': 0, 'B': 1}, umap_project=True)
    with pytest.raises(NotImplementedError, match='fit_pca'):
        load_dataset_from_precomputed('nowhere', 'nothing', umap_project=True)


def test_entry_points_refuse_bad_arguments_before_any_device_work():
    from multimodaltopicsegmentation_amd import _lib as L
    buf = (C.c_double * 16)()
    p = C.addressof(buf)                                             # a non-null HOST address: a refused call never reads it
    lib = L.lib
    # null pointers
    assert lib.mts_pca_colsum(None, L.F32, 4, 4, None, p) == 1 and lib.mts_pca_colsum(None, L.F32, 4, 4, p, None) == 1
    assert lib.mts_pca_gram(None, L.BF16, 4, 4, None, p, p) == 1 and lib.mts_pca_gram(None, L.BF16, 4, 4, p, None, p) == 1
    assert lib.mts_pca_gram(None, L.F32, 4, 4, p, p, None) == 1
    for hole in range(4):
        args = [p, p, p, p]
        args[hole] = None
        assert lib.mts_pca_project(None, L.F32, L.F32, 4, 4, 2, *args) == 1, hole
    # sizes
    for rows, D in ((0, 4), (-1, 4), (4, 0), (4, -3)):
        assert lib.mts_pca_colsum(None, L.F32, rows, D, p, p) == 1
        assert lib.mts_pca_gram(None, L.F32, rows, D, p, p, p) == 1
        assert lib.mts_pca_project(None, L.F32, L.F32, rows, D, 1, p, p, p, p) == 1
    for k in (0, -1, 5):
        assert lib.mts_pca_project(None, L.BF16, L.BF16, 4, 4, k, p, p, p, p) == 1
    # dtypes
    assert lib.mts_pca_colsum(None, 7, 4, 4, p, p) == 1 and lib.mts_pca_gram(None, -1, 4, 4, p, p, p) == 1
    assert lib.mts_pca_project(None, L.F32, 2, 4, 4, 2, p, p, p, p) == 1
    with pytest.raises(ValueError):
        L.check(lib.mts_pca_project(None, L.F32, 2, 4, 4, 2, p, p, p, p))
    # outside what the kernels cover
    assert lib.mts_pca_colsum(None, L.F32, 4, 4097, p, p) == 2
    assert lib.mts_pca_gram(None, L.F32, 4, 4097, p, p, p) == 2
    assert lib.mts_pca_project(None, L.F32, L.BF16, 4, 4097, 2, p, p, p, p) == 2
    assert lib.mts_pca_project(None, L.BF16, L.F32, 4, 4, 2, p, p, p, p) == 2
    with pytest.raises(NotImplementedError):
        L.check(lib.mts_pca_gram(None, L.F32, 4, 4097, p, p, p))
