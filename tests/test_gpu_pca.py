"""PCA projection on the GPU (csrc/pca.hip, pca.py, ResidentCorpus.fit_pca / projected).

Exact tests carry the weight against indexing, tail, mirror and fold mistakes: integers in -8 .. 8 about integer centres in -2 .. 2 (and
integer components in -3 .. 3) keep every product and partial sum below 2^24, so the fp32 matrix instruction, the fp64 fold and the one
rounding to bf16 are exact and the comparison is torch.equal, on outputs prefilled with a sentinel.  The rounding tests use real data
about a real centre and bounds that follow from the arithmetic the header states (an fma chain of at most PCA_SLICE terms in the Gram
matrix, of D terms in the projection, plus the centring), never from what the kernels give; the end-to-end test has no chosen tolerance
at all: the eigenvalues and components may differ from the oracle's by what Weyl's and Davis-Kahan's theorems allow for the measured
difference of the two scatter matrices.

Largest ratios of error to bound measured on an MI355X (printed by the rounding test): Gram 0.015 (fp32 storage) / 0.10 (bf16),
projection 0.028 / 0.97 / 0.97 (fp32 -> fp32, bf16 -> bf16, fp32 -> bf16: a bf16 output's one rounding is up to 2^-8 of the value and is
the whole of it), column sums 0 (exact in fp64 at these sizes)."""
import numpy as np
import pytest
import torch

from tests import pca_oracle as O
from tests.test_pca_cpu import K, corpus_of

pytestmark = pytest.mark.gpu
DEV = 'cuda'
F32, BF16 = torch.float32, torch.bfloat16
PCA_SLICE = 1024                                 # rows between two folds of the Gram kernel's fp32 accumulators (csrc/pca.hip), as built
PCA_TILE = 64                                    # edge of a workgroup's output tile (csrc/pca.hip), as built
SENTINEL = -12288.0                              # exact in bf16 too; no expected value equals it

GRAM_D = sorted({1, 3, 16, 63, 64, 65, 130, PCA_TILE + 1})
GRAM_ROWS = [1, 2, 63, 64, 65, PCA_SLICE - 1, PCA_SLICE, PCA_SLICE + 1, 2 * PCA_SLICE + 188]
PROJ_ROWS = [1, 63, 65, 300]
PROJ_D = [1, 3, 65, 130]
PAIRS = [(F32, F32), (BF16, BF16), (F32, BF16)]
U32 = 2.0 ** -24                                 # unit roundoff of fp32
U_BF16 = 2.0 ** -8                               # unit roundoff of bf16 (8 significand bits, round to nearest even)


def _dev(a, dtype=F32):
    return torch.from_numpy(np.array(a, order='C')).to(dtype).to(DEV)                      # a copy: the corpora are read-only


def _integer(rows, D):
    """the leading [rows, D] block of ONE integer corpus (made once): every shape sees other tails of the same data"""
    return np.ascontiguousarray(O.integer_matrix(GRAM_ROWS[-1], 130)[:rows, :D])


# ---- exact: column sums and the Gram matrix ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', [F32, BF16], ids=['fp32', 'bf16'])
@pytest.mark.parametrize('D', GRAM_D)
def test_colsum_and_gram_are_exact_on_integers(D, dtype):
    from multimodaltopicsegmentation_amd import ops
    c = np.ascontiguousarray(O.integer_center(130)[:D])
    cd = _dev(c)
    for rows in GRAM_ROWS:
        x = _integer(rows, D)
        xd = _dev(x, dtype)
        s = torch.full((D,), SENTINEL, dtype=torch.float64, device=DEV)
        g = torch.full((D, D), SENTINEL, dtype=torch.float64, device=DEV)
        assert ops.pca_colsum(xd, s) is s and ops.pca_gram(xd, cd, g) is g
        want = O.gram(x, c)
        assert np.abs(want).max() < 2 ** 24
        assert np.array_equal(s.cpu().numpy(), O.colsum(x)), (rows, D)
        got = g.cpu()
        assert torch.equal(got, got.T.contiguous()), (rows, D)                       # symmetric bit for bit
        assert np.array_equal(got.numpy(), want), (rows, D)


def test_gram_and_colsum_give_the_same_bits_every_call():
    from multimodaltopicsegmentation_amd import ops
    x = _dev(O.real_matrix(GRAM_ROWS[-1], 130))
    c = (ops.pca_colsum(x) / x.shape[0]).to(F32)
    first = ops.pca_gram(x, c)
    assert torch.equal(ops.pca_gram(x, c), first) and torch.equal(first, first.T.contiguous())
    assert torch.equal(ops.pca_colsum(x), ops.pca_colsum(x))


# ---- exact: the projection -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('pair', PAIRS, ids=['fp32-fp32', 'bf16-bf16', 'fp32-bf16'])
@pytest.mark.parametrize('D', PROJ_D)
def test_projection_is_exact_on_integers(D, pair):
    from multimodaltopicsegmentation_amd import ops
    tin, tout = pair
    c = np.ascontiguousarray(O.integer_center(130)[:D])
    cd = _dev(c)
    for k in sorted({k for k in (1, 2, 9, 65, min(D, 167)) if k <= D}):
        w = O.integer_weights(k, D)
        wd = _dev(w)
        for rows in PROJ_ROWS:
            x = _integer(rows, D)
            want = O.project(x, c, w)
            assert np.abs(want).max() <= 3900
            y = torch.full((rows, k), SENTINEL, dtype=tout, device=DEV)
            assert ops.pca_project(_dev(x, tin), cd, wd, y) is y
            assert torch.equal(y.cpu(), torch.from_numpy(want).to(F32).to(tout)), (rows, D, k)
    if tin == tout:                                                                  # the default output is the input's dtype
        assert ops.pca_project(_dev(x, tin), cd, wd).dtype == tin
    else:
        with pytest.raises(NotImplementedError):
            ops.pca_project(_dev(x, BF16), cd, wd, torch.empty((rows, k), dtype=F32, device=DEV))


# ---- rounding ------------------------------------------------------------------------------------------------------------------------
def test_rounding_stays_inside_the_bounds_of_the_stated_arithmetic():
    """real data whose column means are many times their spread, about the product's own centre fp32(colsum / N).  Gram: an fma chain
    of PCA_SLICE terms plus the two centring roundings; projection: a chain of D terms, plus one bf16 rounding for a bf16 output;
    column sums: rows additions in fp64.  A kernel that accumulates the whole corpus in fp32 can exceed the Gram bound; a correct one
    cannot."""
    from multimodaltopicsegmentation_amd import ops
    rows, D = GRAM_ROWS[-1], 130
    x32 = O.real_matrix(rows, D)
    w = np.linalg.qr(np.random.default_rng(31).standard_normal((D, K)))[0].T.astype(np.float32)
    ratios = {}
    for name, dtype in (('fp32', F32), ('bf16', BF16)):
        xd = _dev(x32, dtype)
        x = xd.to(F32).cpu().numpy()                                                 # the corpus as stored
        s = ops.pca_colsum(xd).cpu().numpy()
        bound = rows * 2.0 ** -53 * np.abs(x.astype(np.float64)).sum(axis=0)
        err = np.abs(s - O.colsum(x))
        ratios['colsum ' + name] = float((err / bound).max())
        assert (err <= bound).all()
        c = (s / rows).astype(np.float32)
        g = ops.pca_gram(xd, _dev(c)).cpu().numpy()
        bound = (PCA_SLICE + 4) * U32 * O.gram_abs(x, c)
        err = np.abs(g - O.gram(x, c))
        ratios['gram ' + name] = float((err / bound).max())
        assert (err <= bound).all()
    for tin, tout in PAIRS:
        xd = _dev(x32, tin)
        x = xd.to(F32).cpu().numpy()
        c = (O.colsum(x) / rows).astype(np.float32)
        y = ops.pca_project(xd, _dev(c), _dev(w), torch.empty((rows, K), dtype=tout, device=DEV)).to(torch.float64).cpu().numpy()
        want = O.project(x, c, w)
        bound = (D + 4) * U32 * O.project_abs(x, c, w) + (U_BF16 * np.abs(want) if tout == BF16 else 0.0)
        err = np.abs(y - want)
        ratios[f'project {tin}->{tout}'] = float((err / bound).max())
        assert (err <= bound).all()
    print('largest error / bound:', ratios)


# ---- end to end: no chosen tolerance ---------------------------------------------------------------------------------------------------
_corpora = {}


def _planted(wire):
    if wire not in _corpora:
        _corpora[wire] = corpus_of(O.planted_matrix(), O.PLANTED_ROWS, DEV, wire=wire, segments=True)
    return _corpora[wire]


@pytest.mark.parametrize('wire', ['fp32', 'bf16'])
def test_fit_pca_is_within_the_perturbation_bounds_of_its_own_moments(wire):
    x = O.planted_matrix()                                                           # integers: the bf16 corpus holds the same values
    n, D = x.shape
    corpus = _planted(wire)
    assert corpus.corpus.dtype == (BF16 if wire == 'bf16' else F32)
    r, m = corpus.fit_pca(K, return_moments=True)
    assert set(m) == {'n', 'colsum', 'center', 'gram'} and m['n'] == n and m['center'].dtype == np.float32
    assert np.array_equal(m['colsum'], O.colsum(x)) and np.array_equal(m['center'], (O.colsum(x) / n).astype(np.float32))
    f = O.fit(x, K)
    lam = f['spectrum']
    E = np.linalg.norm(O.scatter_from_moments(n, m['colsum'], m['center'], m['gram']) - O.scatter(x), 2)
    print('||E||_2 =', E)
    assert (np.abs(r.explained_variance_ - f['explained_variance']) <= E / (n - 1) + 1e-12 * lam[0]).all()            # Weyl
    assert O.sign_rule_holds(r.components_)
    for j in range(K):                                                                                                # Davis-Kahan
        gap = np.abs(np.delete(lam, j) - lam[j]).min()
        d = min(np.linalg.norm(r.components_[j] - f['components'][j]), np.linalg.norm(r.components_[j] + f['components'][j]))
        assert d <= 2 * np.sqrt(2) * E / ((n - 1) * gap) + 1e-9, j
    assert (r.n_components_, r.n_samples_, r.n_features_in_) == (K, n, D)
    assert np.abs(r.mean_ - f['mean']).max() <= 1e-12
    again = corpus.fit_pca(K)                                                        # the same bits every time
    for key, v in r.state_dict().items():
        assert np.array_equal(v, again.state_dict()[key]), key


# ---- transform and projected ---------------------------------------------------------------------------------------------------------
def _projection_bound(x, r, out_dtype):
    """(oracle projection of the stored rows x under reducer r's fp32 operands, its rounding bound)"""
    c, w = r.mean_.astype(np.float32), r.components_.astype(np.float32)
    want = O.project(x, c, w)
    return want, (x.shape[1] + 4) * U32 * O.project_abs(x, c, w) + (U_BF16 * np.abs(want) if out_dtype == BF16 else 0.0)


@pytest.mark.parametrize('wire', ['fp32', 'bf16'])
def test_projected_corpus_and_transform_agree_with_the_oracle_and_each_other(wire):
    corpus = _planted(wire)
    x = corpus.corpus.to(F32).cpu().numpy()
    r = corpus.fit_pca(K)
    P = corpus.projected(r)
    assert P is not corpus and P.corpus.shape == (x.shape[0], K) and P.corpus.dtype == corpus.wire and P.corpus.is_contiguous()
    assert P.targets is corpus.targets and P.row_start is corpus.row_start and P.corpus2 is None and P._ring is None
    assert corpus.corpus.shape[1] == O.PLANTED_D                                    # the parent is untouched
    want, bound = _projection_bound(x, r, corpus.wire)
    assert (np.abs(P.corpus.to(torch.float64).cpu().numpy() - want) <= bound).all()
    whole = r.transform(corpus.corpus)
    assert torch.equal(whole, P.corpus)
    idx = [2, 0, 9, 4, 9]
    parent, got = corpus.batch(idx), P.batch(idx)
    assert set(got) == set(parent)
    assert got['src_tokens'].shape == parent['src_tokens'].shape[:2] + (K,) and got['src_tokens'].dtype == corpus.wire
    assert torch.equal(got['src_lengths'], parent['src_lengths']) and torch.equal(got['tgt_tokens'], parent['tgt_tokens'])
    assert torch.equal(got['id'], parent['id']) and got['src_segments'] == parent['src_segments'] and got['src_tokens2'] is None
    after = r.transform(parent['src_tokens'])                                        # [B, Lmax, D] -> [B, Lmax, K]
    assert after.shape == got['src_tokens'].shape
    for b, n in enumerate(parent['src_lengths'].tolist()):
        assert torch.equal(after[b, :n], got['src_tokens'][b, :n]), b               # bitwise on the real rows
        assert not got['src_tokens'][b, n:].any()                                   # the pad of a projected batch is 0
    # a state round trip projects to the same bits
    from multimodaltopicsegmentation_amd import PcaReducer
    assert torch.equal(PcaReducer.from_state_dict(r.state_dict()).transform(corpus.corpus), P.corpus)
    with pytest.raises(ValueError):
        P.projected(r)                                                               # width K is not the reducer's


def test_second_input_is_fitted_and_projected_on_request():
    x = O.planted_matrix()
    second = np.ascontiguousarray(O.integer_matrix(x.shape[0], 21, seed=1))
    corpus = corpus_of(x, O.PLANTED_ROWS, DEV, second=second)
    r1, r2 = corpus.fit_pca(K), corpus.fit_pca(5, field='embeddings2')
    assert r2.n_features_in_ == 21 and r2.n_components_ == 5
    only_first, both = corpus.projected(r1), corpus.projected(r1, r2)
    assert only_first.corpus2 is corpus.corpus2 and both.corpus2.shape == (x.shape[0], 5)
    want, bound = _projection_bound(second, r2, F32)
    assert (np.abs(both.corpus2.to(torch.float64).cpu().numpy() - want) <= bound).all()
    assert torch.equal(both.corpus, only_first.corpus)
    b = both.batch([1, 2])
    assert b['src_tokens'].shape[2] == K and b['src_tokens2'].shape[2] == 5
    with pytest.raises(ValueError):
        corpus.projected(r1, r1)


# ---- the pipeline on a projected corpus ----------------------------------------------------------------------------------------------
def test_augmented_and_masked_views_of_a_projected_corpus_equal_gather_then_project():
    corpus = _planted('fp32')
    r = corpus.fit_pca(K)
    P = corpus.projected(r)
    idx = [2, 5, 9]
    pairs = [(corpus.augmented('reverse').batch([i + len(corpus) for i in idx]), P.augmented('reverse').batch([i + len(corpus) for i in idx])),
             (corpus.masked(0.5, seed=4).batch(idx), P.masked(0.5, seed=4).batch(idx))]
    for first, got in pairs:
        assert torch.equal(first['src_lengths'], got['src_lengths']) and torch.equal(first['tgt_tokens'], got['tgt_tokens'])
        assert first['src_segments'] == got['src_segments'] and got['src_tokens'].shape[2] == K
        after = r.transform(first['src_tokens'])
        for b, n in enumerate(first['src_lengths'].tolist()):
            assert 0 < n < corpus.rows[idx[b]]                                       # the view did reorder / drop rows
            want, bound = _projection_bound(first['src_tokens'][b, :n].cpu().numpy(), r, F32)
            assert (np.abs(got['src_tokens'][b, :n].to(torch.float64).cpu().numpy() - want) <= bound).all()
            assert (np.abs((after[b, :n] - got['src_tokens'][b, :n]).to(torch.float64).cpu().numpy()) <= 2 * bound).all()


def test_fit_and_evaluate_run_on_projected_folds():
    from multimodaltopicsegmentation_amd import BiLSTM, evaluate, fit, project_folds
    from multimodaltopicsegmentation_amd.trainer import NativeTrainer
    x = O.planted_matrix()
    cut = np.concatenate([[0], np.cumsum(O.PLANTED_ROWS)])
    parts = {'train': (0, 8), 'val': (8, 9), 'test': (9, 11)}                        # documents 0..7, 8, 9..10
    train, val, test = (corpus_of(np.ascontiguousarray(x[cut[a]:cut[b]]), O.PLANTED_ROWS[a:b], DEV) for a, b in parts.values())
    ((ptrain, pval, ptest),), (r,) = project_folds([(train, val, test)], n_components=K)
    assert r.n_samples_ == int(cut[8]) and np.array_equal(r.state_dict()['components_'], train.fit_pca(K).components_)
    assert ptrain.corpus.shape[1] == pval.corpus.shape[1] == ptest.corpus.shape[1] == K
    assert torch.equal(ptest.corpus, r.transform(test.corpus))                       # the train split's reducer on the test split
    model = BiLSTM(2, K, 16, num_layers=1, loss_fn='FocalLoss', compute_dtype='fp32', seed=11).to(DEV)
    trainer = NativeTrainer(model, lr=1e-3)
    record = fit(trainer, ptrain, pval, batch_size=4, max_epochs=2)
    assert len(record['epochs']) == 2 and all(np.isfinite(e['train_loss']) and np.isfinite(e['val_loss']) for e in record['epochs'])
    out = evaluate(trainer, ptest, batch_size=4)
    assert len(out['documents']) == 2 and all(np.isfinite(v) for v in out['mean'].values())


def test_projected_folds_go_to_cross_validate_unchanged():
    from multimodaltopicsegmentation_amd import BiLSTM, cross_validate, project_folds
    from multimodaltopicsegmentation_amd.trainer import NativeTrainer
    x = O.planted_matrix()
    cut = np.concatenate([[0], np.cumsum(O.PLANTED_ROWS)])

    def part(a, b):
        return corpus_of(np.ascontiguousarray(x[cut[a]:cut[b]]), O.PLANTED_ROWS[a:b], DEV)
    folds = [(part(0, 8), part(8, 9), part(9, 11)), (part(3, 11), None, part(0, 3))]
    projected, reducers = project_folds(folds, n_components=K)
    assert [r.n_samples_ for r in reducers] == [int(cut[8]), int(cut[11] - cut[3])]
    assert projected[1][1] is None and all(c.corpus.shape[1] == K for f in projected for c in f if c is not None)
    out = cross_validate(lambda: NativeTrainer(BiLSTM(2, K, 16, num_layers=1, loss_fn='FocalLoss', compute_dtype='fp32', seed=11).to(DEV), lr=1e-3),
                         projected, samples=200, batch_size=4, max_epochs=1)
    assert len(out['folds']) == 2 and all(np.isfinite(v['mean']) for v in out['report'].values())
