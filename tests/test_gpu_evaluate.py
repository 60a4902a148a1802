"""GPU tests of the test pass (evaluate.evaluate / NativeTrainer.evaluate / cross_validate) on tiny fp32 models and the 12-document
corpora of tests/test_gpu_fit.py: every per-document float equals the host metrics over the boundary lists the tagger's own forward
returns for the batches evaluate forms, the means equal TextSegmenter.test_step's, two ranks agree with one process, and the driver over
folds is fit followed by evaluate."""
import functools
import os
import socket

import numpy as np
import pytest
import torch

from tests.test_gpu_fit import BATCH, DEV, SEED, TRAIN_LENGTHS, VAL_LENGTHS, _build, _corpus

pytestmark = pytest.mark.gpu
TEST_LENGTHS = [9, 33, 5, 27, 14, 40, 6, 19, 11, 36, 8, 23]
KINDS = ['bilstm', 'transformer', 'latefusion', 'sheikh', 'crf_viterbi', 'crf_marginal']
METRICS = ('Pk', 'WD', 'F1', 'b_precision', 'b_recall', 'b_f1')


def _model(kind):
    from multimodaltopicsegmentation_amd import BiRnnCrf, SheikhBiLSTM
    if kind == 'sheikh':                                 # dropout_in 0: the reference's 0.5 is live in eval mode too and would differ call to call
        return SheikhBiLSTM(2, 64, 32, 1, dropout_in=0.0, compute_dtype='fp32', seed=11).to(DEV)
    if kind.startswith('crf'):
        return BiRnnCrf(2, 64, 32, num_layers=1, architecture='rnn', compute_dtype='fp32', seed=11, decode=kind[4:]).to(DEV)
    return _build(kind)


def _corpus_of(kind, lengths, seed):
    return _corpus(kind if kind in ('bilstm', 'transformer', 'latefusion') else 'bilstm', lengths, seed)


@functools.lru_cache(maxsize=None)
def _fitted(kind):
    """-> (model, the threshold its fit chose); the three kinds of tests/test_gpu_fit.py are trained for two epochs with the search on"""
    from multimodaltopicsegmentation_amd.trainer import NativeTrainer
    model = _model(kind).eval()
    if kind not in ('bilstm', 'transformer', 'latefusion'):
        return model, 0.5
    out =NativeTrainer(model, lr=1e-3).fit(_corpus_of(kind, TRAIN_LENGTHS, 2), _corpus_of(kind, VAL_LENGTHS, 6), batch_size=BATCH, max_epochs=2,
                                            seed=SEED, search_threshold=True, metric='Pk')
    assert model.th == out['threshold'] and out['threshold'] is not None
    return model, out['threshold']


def _own_forward(model, batch):
    """(scores, boundary lists) by the tagger's own forward"""
    if batch.get('src_tokens2') is not None:
        return model(batch['src_tokens'], batch['src_tokens2'], batch['src_lengths'])
    return model(batch['src_tokens'], batch['src_lengths'])


def _winpr_on_host(tag, tgt, end_boundary, k=10):
    """metrics.WinPR as test_step's scaiano branch calls it, in integers; (0, 0, 0) where it divides by zero (the sweep's stated convention)"""
    from multimodaltopicsegmentation_amd import metrics
    tag, tgt = [int(v) for v in tag], [int(v) for v in tgt]
    if end_boundary:
        tag[-1] = 0
        tgt[-1] = 0
    try:
        return tuple(float(v) for v in metrics.WinPR(tag, tgt, k))
    except ZeroDivisionError:
        return 0.0, 0.0, 0.0


def _host_rows(model, corpus, docs, batch_size, th, end_boundary, zero=False):
    """{document: the six floats} from the boundary lists of the tagger's own forward at ``th`` over the batches evaluate forms"""
    from multimodaltopicsegmentation_amd.threshold_search import host_metrics
    had, old = hasattr(model, 'th'), getattr(model, 'th', None)
    model.th = th
    rows = {}
    try:
        for s in range(0, len(docs), batch_size):
            idx = docs[s:s + batch_size]
            batch = corpus.batch(idx)
            lens = batch['src_lengths'].tolist()
            tags = [[0] * n for n in lens] if zero else _own_forward(model, batch)[1]
            tgt = batch['tgt_tokens'].cpu().numpy()
            for b, doc in enumerate(idx):
                tag = [int(v) for v in tags[b]]
                assert len(tag) == lens[b]
                rows[doc] = host_metrics(tag, tgt[b, :lens[b]], end_boundary) + _winpr_on_host(tag, tgt[b, :lens[b]], end_boundary)
    finally:
        if had:
            model.th = old
        else:
            del model.th
    return rows


def _check_against_rows(ev, rows):
    n = len(rows)
    assert ev['documents'].tolist() == sorted(rows) and ev['documents'].dtype == np.int64
    for j, name in enumerate(METRICS):
        col = ev['per_document'][name]
        assert col.dtype == np.float64 and col.shape == (n,)
        assert col.tolist() == [rows[d][j] for d in sorted(rows)], name
        acc = 0.0
        for v in col.tolist():                           # one document after the other
            acc = acc + v
        assert ev['mean'][name] == acc / n and isinstance(ev['mean'][name], float), name
    assert ev['counts']['sweep'].shape == (n, 6) and ev['counts']['winpr'].shape == (n, 3)
    assert ev['counts']['sweep'].dtype == np.int64 and ev['counts']['winpr'].dtype == np.int64


def _same(a, b):
    if isinstance(a, dict):
        return isinstance(b, dict) and list(a) == list(b) and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    if isinstance(a, np.ndarray):
        return isinstance(b, np.ndarray) and a.dtype == b.dtype and np.array_equal(a, b)
    return a == b


@pytest.mark.parametrize('end_boundary', [False, True])
@pytest.mark.parametrize('kind', KINDS)
def test_per_document_floats_equal_the_host_metrics_of_the_own_forward(kind, end_boundary):
    from multimodaltopicsegmentation_amd import evaluate
    model, chosen = _fitted(kind)
    test = _corpus_of(kind, TEST_LENGTHS, 8)
    docs = list(range(len(test)))
    mixed = 0
    for th in (0.4, chosen):
        ev = evaluate(model, test, batch_size=5, threshold=th, end_boundary=end_boundary)         # batches of 5, 5 and 2 documents
        assert ev['threshold'] == (0.5 if kind == 'crf_viterbi' else th)
        assert set(ev) == {'threshold', 'documents', 'per_document', 'mean', 'counts'}
        _check_against_rows(ev, _host_rows(model, test, docs, 5, th, end_boundary))
        mixed += int((ev['counts']['sweep'][:, 3:5].sum(axis=1) > 0).any())
    # threshold=None reads model.th (the fit's, where there was one), else 0.4
    assert evaluate(model, test, batch_size=5, end_boundary=end_boundary)['threshold'] == \
        (0.5 if kind == 'crf_viterbi' else getattr(model, 'th', None) or 0.4)
    print(kind, 'thresholds with a predicted boundary:', mixed)


@pytest.mark.parametrize('end_boundary', [False, True])
def test_means_equal_test_step_for_pk_wd_f1(end_boundary):
    from multimodaltopicsegmentation_amd import TextSegmenter, evaluate
    torch.manual_seed(3)
    test = _corpus('bilstm', TEST_LENGTHS, 8)
    ts = TextSegmenter(2, 64, 32, architecture='BiLSTM', loss_fn='FocalLoss', compute_dtype='fp32', threshold=0.5, metric='Pk',
                       end_boundary=end_boundary).to(DEV).eval()
    res = ts.test_step(test.batch(list(range(len(test)))), 0)
    ev = evaluate(ts, test, batch_size=len(test), threshold=0.5, end_boundary=end_boundary)
    print('test_step', res, 'evaluate', ev['mean'])
    assert (ev['mean']['Pk'], ev['mean']['WD'], ev['mean']['F1'], ev['threshold']) == \
        (res['test_loss'], res['WD_loss'], res['F1_loss'], res['threshold'])
    assert 0 < ev['mean']['Pk'] < 1


def _scaiano_pair():
    """(test_step's dict under metric 'scaiano', evaluate's result) for one model object over all twelve documents in one batch, at the
    highest threshold of a short list at which metrics.WinPR divides by zero for no document: every document has TP > 0, or TP + FP == 0,
    where upstream reports zeros as the sweep does"""
    from multimodaltopicsegmentation_amd import TextSegmenter, evaluate
    torch.manual_seed(3)
    test = _corpus('bilstm', TEST_LENGTHS, 8)
    ts = TextSegmenter(2, 64, 32, architecture='BiLSTM', loss_fn='FocalLoss', compute_dtype='fp32', threshold=0.5, metric='scaiano').to(DEV).eval()
    for th in (0.5, 0.45, 0.4, 0.3, 0.2, 0.1, 0.05):
        ev = evaluate(ts, test, batch_size=len(test), threshold=th)
        c = ev['counts']['winpr']
        if ((c[:, 0] > 0) | (c[:, 0] + c[:, 1] == 0)).all():
            break
    else:
        raise AssertionError('no threshold of the list leaves every document a defined WinPR')
    ts.threshold = th
    res = ts.test_step(test.batch(list(range(len(test)))), 0)
    assert res['threshold'] == ev['threshold'] == th and (c[:, 0] > 0).sum() >= 6
    return res, ev


def test_means_equal_test_step_for_scaiano():
    """``==`` between evaluate's means and the dict test_step returns under metric 'scaiano'.  test_step hands metrics.WinPR the target as
    a float32 array, so WinPR's quotients, test_step's running sums and its means are numpy.float32
    (tests/test_gpu_winpr_sweep.py::test_relation_to_test_step_in_float32 states that relation), whereas evaluate takes its floats from the
    integers in float64 through winpr_floats.  numpy compares a python float with a numpy.float32 in float32, so this ``==`` says that the
    float64 means round to test_step's float32 ones; test_scaiano_means_are_test_step_s_up_to_its_float32_arithmetic bounds the float64
    difference itself from the formats."""
    res, ev = _scaiano_pair()
    print('test_step', {k: repr(v) for k, v in res.items()}, 'evaluate', ev['mean'])
    assert (ev['mean']['b_precision'], ev['mean']['b_recall'], ev['mean']['b_f1']) == (res['b_precision'], res['b_recall'], res['test_loss'])


def test_scaiano_means_are_test_step_s_up_to_its_float32_arithmetic():
    """Each of test_step's per-document WinPR values is within 8 * 2**-24 of the float64 one (six float32 roundings of values <= 1, the
    bound of test_relation_to_test_step_in_float32); its float32 running sum over n = 12 documents stays below 16, so each of the 11
    additions rounds by at most half an ulp of [8, 16), 2**-21; the division by n adds one rounding of a value <= 1, 2**-25."""
    res, ev = _scaiano_pair()
    n = len(TEST_LENGTHS)
    bound = 8 * 2.0 ** -24 + (n - 1) * 2.0 ** -21 / n + 2.0 ** -25
    for name, key in (('b_precision', 'b_precision'), ('b_recall', 'b_recall'), ('b_f1', 'test_loss')):
        assert abs(ev['mean'][name] - float(res[key])) <= bound, (name, ev['mean'][name], res[key])


def test_baseline_falsy_threshold_scores_and_the_training_flag():
    from multimodaltopicsegmentation_amd import evaluate
    model, _ = _fitted('bilstm')
    test = _corpus('bilstm', TEST_LENGTHS, 8)
    docs = list(range(len(test)))
    # the all-zero hypothesis: no forward, threshold reported as 0.4
    base = evaluate(model, test, batch_size=5, zero_baseline=True)
    assert base['threshold'] == 0.4
    _check_against_rows(base, _host_rows(model, test, docs, 5, 0.4, False, zero=True))
    tgt = [test.batch([d])['tgt_tokens'].cpu().numpy()[0] for d in docs]
    assert (base['counts']['sweep'][:, 3:5] == 0).all()                                          # tp, fp
    assert base['counts']['sweep'][:, 5].tolist() == [int((t[:-1] == 1).sum()) for t in tgt]      # fn: the target's boundaries but its last sentence
    assert (base['counts']['winpr'][:, 0] == 0).all() and all(base['mean'][k] == 0.0 for k in ('F1', 'b_precision', 'b_recall', 'b_f1'))
    # threshold=0 means 0.5
    half, zero = evaluate(model, test, batch_size=5, threshold=0.5), evaluate(model, test, batch_size=5, threshold=0)
    assert zero['threshold'] == 0.5 and _same(zero, half)
    assert not _same(half, base)
    # return_scores: every document's scores trimmed to its length, and nothing else changes
    kept = evaluate(model, test, batch_size=5, threshold=0.5, return_scores=True)
    scores = kept.pop('scores')
    assert _same(kept, half) and len(scores) == len(test)
    for s in range(0, len(docs), 5):
        idx = docs[s:s + 5]
        batch = test.batch(idx)
        own = _own_forward(model, batch)[0].cpu().numpy()
        for b, d in enumerate(idx):
            n = int(batch['src_lengths'][b])
            assert scores[d].dtype == np.float32 and scores[d].shape == (n, own.shape[2]) and np.array_equal(scores[d], own[b, :n])
    # the training flag is restored, whichever it was
    for flag in (True, False):
        model.train(flag)
        evaluate(model, test, batch_size=12, threshold=0.5)
        assert model.training is flag
    model.eval()


# ---- two ranks ----------------------------------------------------------------------------------------------------------------
DP_TEST = {'five': TEST_LENGTHS[:5], 'one': TEST_LENGTHS[:1]}      # 3 + 2 documents; 1 + 0: the second rank scores nothing and still joins in
DP_RUNS = [('five', False), ('five', True), ('one', False)]


def _dp_worker(rank, world, port, out_dir):
    import torch.distributed as dist
    from multimodaltopicsegmentation_amd.trainer import NativeTrainer
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    torch.cuda.set_device(0)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    out = []
    for name, end_boundary in DP_RUNS:
        trainer = NativeTrainer(_build('bilstm'), lr=1e-3)
        out.append(trainer.evaluate(_corpus('bilstm', DP_TEST[name], 8), batch_size=2, threshold=0.5, end_boundary=end_boundary))
    torch.save(out, os.path.join(out_dir, f'r{rank}.pt'))
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_score_their_own_documents_and_agree(tmp_path):
    import time
    import torch.multiprocessing as mp
    from multimodaltopicsegmentation_amd import evaluate
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.spawn(_dp_worker, args=(2, port, str(tmp_path)), nprocs=2, join=False)
    deadline = time.monotonic() + 240
    try:
        while not ctx.join(timeout=5):                            # raises when a rank exits with a non-zero status
            assert time.monotonic() < deadline, 'the two ranks did not finish in 240 s'
    finally:
        for p in ctx.processes:
            if p.is_alive():
                p.kill()
    r0, r1 = (torch.load(os.path.join(tmp_path, f'r{r}.pt'), weights_only=False) for r in range(2))
    for (name, end_boundary), a, b in zip(DP_RUNS, r0, r1):
        alone = evaluate(_build('bilstm'), _corpus('bilstm', DP_TEST[name], 8), batch_size=2, threshold=0.5, end_boundary=end_boundary)
        assert _same(a, b) and _same(a, alone), name
        assert a['documents'].tolist() == list(range(len(DP_TEST[name])))


# ---- the driver over folds -------------------------------------------------------------------------------------------------------
def test_cross_validate_is_fit_then_evaluate_per_fold():
    from multimodaltopicsegmentation_amd import bootstrap_ci, cross_validate
    from multimodaltopicsegmentation_amd.trainer import NativeTrainer
    folds = [(_corpus('bilstm', TRAIN_LENGTHS, 2), _corpus('bilstm', VAL_LENGTHS, 6), _corpus('bilstm', TEST_LENGTHS, 8)),
             (_corpus('bilstm', VAL_LENGTHS, 6), _corpus('bilstm', TEST_LENGTHS, 8), _corpus('bilstm', TRAIN_LENGTHS, 2))]
    kw = dict(batch_size=BATCH, max_epochs=2, seed=SEED, search_threshold=True, metric='F1')
    out = cross_validate(lambda: NativeTrainer(_build('bilstm'), lr=1e-3), folds, samples=2000, bootstrap_seed=4, **kw)
    assert set(out) == {'folds', 'fold_means', 'report', 'pooled'} and len(out['folds']) == 2
    assert all(set(f) == {'fit', 'test'} and len(f['fit']['epochs']) == 2 for f in out['folds'])
    # fold 0 by hand on a twin
    twin = NativeTrainer(_build('bilstm'), lr=1e-3)
    record = twin.fit(folds[0][0], folds[0][1], **kw)
    by_hand = twin.evaluate(folds[0][2], batch_size=BATCH)
    assert out['folds'][0]['fit'] == record and _same(out['folds'][0]['test'], by_hand)
    assert by_hand['threshold'] == record['threshold'] == twin.model.th
    assert set(out['fold_means']) == set(METRICS) == set(out['report']) == set(out['pooled'])
    for k in METRICS:
        assert out['fold_means'][k].shape == (2,) and out['fold_means'][k].tolist() == [f['test']['mean'][k] for f in out['folds']]
    ci = bootstrap_ci(out['fold_means'], samples=2000, seed=4)
    pooled = bootstrap_ci({k: np.concatenate([f['test']['per_document'][k] for f in out['folds']]) for k in METRICS}, samples=2000, seed=4)
    for k in METRICS:
        assert out['report'][k] == {stat: ci[stat][k] for stat in ('mean', 'lo', 'hi', 'half_width')}
        assert out['pooled'][k] == {stat: pooled[stat][k] for stat in ('mean', 'lo', 'hi', 'half_width')}
        assert out['report'][k]['lo'] <= out['report'][k]['mean'] <= out['report'][k]['hi']
    # without a validation corpus the fit monitors the training loss and the test pass falls back on 0.4
    alone = cross_validate(lambda: NativeTrainer(_build('bilstm'), lr=1e-3), [(folds[0][0], None, folds[0][2])], samples=64,
                           batch_size=BATCH, max_epochs=1, seed=SEED)
    assert alone['folds'][0]['test']['threshold'] == 0.4 and alone['fold_means']['Pk'].shape == (1,)
    assert alone['report']['Pk']['lo'] == alone['report']['Pk']['hi'] == alone['fold_means']['Pk'][0]
