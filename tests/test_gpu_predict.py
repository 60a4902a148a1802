"""GPU tests of the prediction pass (multimodaltopicsegmentation_amd/predict.py) on tiny fp32 taggers over an UNLABELLED corpus
(ResidentCorpus.from_documents) of 1, 2, 63, 64 and 130 sentences: the tags equal the boundary lists the tagger's own forward returns for
the batches ``predict`` forms, the segment tables follow from them by the header's rule, ``pool`` is ``ops.frame_pool`` on host-built
offsets, ``evaluate(min_segment=3)`` is ``evaluate`` of a stand-in whose scores are the constrained decode's saturated tags, and two ranks
return the single-process ``Prediction``.  Everything is ``==``."""
import os
import socket

import numpy as np
import pytest
import torch

from tests import segment_decode_oracle as O
from tests.test_gpu_evaluate import TEST_LENGTHS, _model, _own_forward, _same
from tests.test_gpu_fit import DEV, _build, _corpus

pytestmark = pytest.mark.gpu
DOC_LENGTHS = (1, 2, 63, 64, 130)
BATCH = 3                                                   # batches of 1 | 2 | 63 and 64 | 130 sentences
NAMES = [f'rec{k}.npy' for k in range(len(DOC_LENGTHS))]
KINDS = ['bilstm', 'transformer', 'sheikh', 'crf_viterbi', 'crf_marginal']


def _documents(seed=21, D=64):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(n, D, generator=g) for n in DOC_LENGTHS]


def _unlabelled():
    from multimodaltopicsegmentation_amd import ResidentCorpus
    return ResidentCorpus.from_documents(_documents(), DEV, names=NAMES)


def _tagger(kind):
    if kind == 'transformer':                               # 130 sentences need more positions than the fit tests' model has
        from multimodaltopicsegmentation_amd import Transformer_segmenter
        return Transformer_segmenter(2, 64, 32, num_layers=2, nheads=4, loss_fn='FocalLoss', window_size=4, compute_dtype='fp32',
                                     max_position_embedding=256, seed=11).to(DEV).eval()
    return _model(kind).eval()


def _median_threshold(model, corpus, kind):
    """a threshold with tags on either side of it: the median of the decode probabilities (1 - it for SheikhBiLSTM's inverted rule)"""
    from multimodaltopicsegmentation_amd import predict
    p = np.concatenate(predict(model, corpus, batch_size=BATCH, threshold=0.5, return_probabilities=True).probabilities)
    mid = float(np.float32(np.median(p)))
    return 1.0 - mid if kind == 'sheikh' else mid


def _as_dict(p):
    return dict(vars(p))


@pytest.mark.parametrize('kind', KINDS)
def test_tags_equal_the_own_forward_and_the_table_follows(kind):
    from multimodaltopicsegmentation_amd import Prediction, predict
    model, corpus = _tagger(kind), _unlabelled()
    assert corpus.labelled is False
    th = 0.5 if kind == 'crf_viterbi' else _median_threshold(model, corpus, kind)
    for close_last in (True, False):
        pred = predict(model, corpus, batch_size=BATCH, threshold=th, close_last=close_last, return_probabilities=True)
        assert isinstance(pred, Prediction) and pred.threshold == th and pred.min_segment == 1 and pred.close_last is close_last
        assert pred.documents.tolist() == [0, 1, 2, 3, 4] and pred.names == NAMES and pred.lengths.tolist() == list(DOC_LENGTHS)
        had = hasattr(model, 'th')
        old = getattr(model, 'th', None)
        model.th = th
        try:
            own = []
            for s in range(0, len(corpus), BATCH):
                own += _own_forward(model, corpus.batch(list(range(s, min(s + BATCH, len(corpus))))))[1]
        finally:
            if had:
                model.th = old
            else:
                del model.th
        mixed = 0
        for d, n in enumerate(DOC_LENGTHS):
            tags = [int(v) for v in own[d]]
            assert len(tags) == n and pred.tags[d].dtype == np.uint8 and pred.tags[d].tolist() == tags, d
            ends, count = O.segment_table(np.array(tags), n, close_last, n)
            assert pred.segment_ends[d].tolist() == ends[:count].tolist() and pred.n_segments[d] == count
            assert pred.probabilities[d].shape == (n,) and pred.probabilities[d].dtype == np.float32
            mixed += int(0 < sum(tags) < n)
        assert mixed >= 2 or kind == 'crf_viterbi', 'the threshold left no document with tags on both sides'
        spans = pred.spans()
        assert all(sp[0][0] == 0 and all(a[1] == b[0] for a, b in zip(sp, sp[1:])) for sp in spans if sp)
        if close_last:
            assert [sp[-1][1] for sp in spans] == list(DOC_LENGTHS)
    # tags and probabilities are read back only when asked for; the table is the same
    bare = predict(model, corpus, batch_size=BATCH, threshold=th, close_last=False)
    assert bare.tags is None and bare.probabilities is None and _same([e for e in bare.segment_ends], [e for e in pred.segment_ends])
    assert model.training is False
    model.train(True)
    predict(model, corpus, batch_size=BATCH, threshold=th)
    assert model.training is True
    model.eval()


def test_minimum_length_decode_in_predict_and_the_viterbi_refusal():
    from multimodaltopicsegmentation_amd import predict
    model, corpus = _tagger('bilstm'), _unlabelled()
    th = _median_threshold(model, corpus, 'bilstm')
    free = predict(model, corpus, batch_size=BATCH, threshold=th, return_probabilities=True)
    for m in (2, 5):
        pred = predict(model, corpus, batch_size=BATCH, threshold=th, min_segment=m, return_probabilities=True)
        assert pred.min_segment == m
        for d, n in enumerate(DOC_LENGTHS):
            assert np.array_equal(pred.probabilities[d].view(np.uint32), free.probabilities[d].view(np.uint32))
            p = pred.probabilities[d]
            want = O.constrained_tags(O.fixed_point(p, th), m, bool(p[-1] > np.float32(th)))
            assert np.array_equal(pred.tags[d], want) and O.admissible(pred.tags[d], m), (m, d)
            assert np.diff(np.concatenate([[0], pred.segment_ends[d]])).min() >= min(m, n)
        assert sum(int(t.sum()) for t in pred.tags) < sum(int(t.sum()) for t in free.tags)        # the constraint bites at the median
    with pytest.raises(ValueError, match='viterbi'):
        predict(_tagger('crf_viterbi'), corpus, min_segment=2)
    with pytest.raises(ValueError):
        predict(model, corpus, min_segment=0)


def test_pool_is_frame_pool_over_the_predicted_segments():
    from multimodaltopicsegmentation_amd import ops, predict
    model, corpus = _tagger('bilstm'), _unlabelled()
    th = _median_threshold(model, corpus, 'bilstm')
    pred = predict(model, corpus, batch_size=BATCH, threshold=th, min_segment=2)
    offsets, doc_of, first = [0], [], 0
    for d, n in enumerate(DOC_LENGTHS):
        offsets += [first + int(e) for e in pred.segment_ends[d]]
        doc_of += [d] * len(pred.segment_ends[d])
        first += n
    assert offsets[-1] == corpus.total_rows and len(offsets) - 1 == int(pred.n_segments.sum())
    start = torch.tensor(offsets, dtype=torch.int64, device=DEV)
    for mode in ('mean', 'max', 'mean_std', 'max_std'):
        got, segment_doc = pred.pool(corpus, mode)
        W = 128 if mode.endswith('_std') else 64
        want = torch.full((len(doc_of), W), float('nan'), dtype=torch.float32, device=DEV)
        ops.frame_pool(corpus.corpus, start, want, first=mode.split('_')[0], with_std=mode.endswith('_std'))
        assert got.dtype == torch.float32 and got.device == corpus.corpus.device and torch.equal(got, want), mode
        assert segment_doc.dtype == np.int64 and segment_doc.tolist() == doc_of
    mean = pred.pool(corpus, 'mean')[0].cpu()
    rows = corpus.corpus.cpu()
    for j in (0, len(doc_of) - 1):
        assert torch.allclose(mean[j], rows[offsets[j]:offsets[j + 1]].mean(dim=0), atol=1e-5)
    with pytest.raises(ValueError, match='close_last'):
        predict(model, corpus, batch_size=BATCH, threshold=th, close_last=False).pool(corpus)
    with pytest.raises(ValueError):
        pred.pool(corpus, 'last')
    with pytest.raises(ValueError):
        pred.pool(corpus, 'mean', field='embeddings2')
    with pytest.raises(ValueError, match='cover'):
        pred.pool(_corpus('bilstm', TEST_LENGTHS, 8))


class _Replay(torch.nn.Module):
    """a stand-in tagger whose scores are stored logits, handed out batch by batch in evaluate's order"""

    def __init__(self, logits):
        super().__init__()
        self.flat = torch.nn.Parameter(torch.zeros(1, device=logits.device))
        self.logits, self.at = logits, 0

    def forward(self, x, lengths):
        B, Lq = x.shape[0], x.shape[1]
        out = self.logits[self.at:self.at + B, :Lq].contiguous()
        self.at += B
        return out, None


def test_evaluate_under_a_minimum_length_and_unchanged_without_it():
    from multimodaltopicsegmentation_amd import evaluate, predict
    model = _build('bilstm').eval()
    test = _corpus('bilstm', TEST_LENGTHS, 8)
    p = np.concatenate(predict(model, test, batch_size=5, threshold=0.5, return_probabilities=True).probabilities)
    th = float(np.float32(np.median(p)))
    plain = evaluate(model, test, batch_size=5, threshold=th)
    assert _same(plain, evaluate(model, test, batch_size=5, threshold=th, min_segment=None))
    assert _same(plain, evaluate(model, test, batch_size=5, threshold=th, min_segment=1))
    for end_boundary in (False, True):
        ev = evaluate(model, test, batch_size=5, threshold=th, min_segment=3, end_boundary=end_boundary, return_scores=True)
        pred = predict(model, test, batch_size=5, threshold=th, min_segment=3, return_tags=True)
        for d, s in enumerate(ev.pop('scores')):
            assert s.shape == (TEST_LENGTHS[d], 1) and np.array_equal(s[:, 0], np.where(pred.tags[d] == 1, np.float32(30), np.float32(-30)))
        twin = evaluate(_Replay(pred.as_saturated(DEV)), test, batch_size=5, threshold=0.5, end_boundary=end_boundary)
        assert ev['threshold'] == th and twin['threshold'] == 0.5
        twin['threshold'] = th
        assert _same(ev, twin)
    assert not _same(ev['counts'], evaluate(model, test, batch_size=5, threshold=th, end_boundary=True)['counts'])
    with pytest.raises(ValueError, match='viterbi'):
        evaluate(_model('crf_viterbi'), test, min_segment=2)
    with pytest.raises(ValueError, match='predict'):
        evaluate(model, _unlabelled())


# ---- two ranks ----------------------------------------------------------------------------------------------------------------
DP_RUNS = [dict(min_segment=1, close_last=True), dict(min_segment=3, close_last=False)]


DP_LENGTHS = (9, 33, 5, 27, 14)                             # 3 + 2 documents; with one document the second rank holds none


def _dp_corpus(n_docs):
    from multimodaltopicsegmentation_amd import ResidentCorpus
    g = torch.Generator().manual_seed(8)
    return ResidentCorpus.from_documents([torch.randn(n, 64, generator=g) for n in DP_LENGTHS[:n_docs]], DEV, names=NAMES[:n_docs])


def _dp_worker(rank, world, port, out_dir):
    import torch.distributed as dist
    from multimodaltopicsegmentation_amd.trainer import NativeTrainer
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    torch.cuda.set_device(0)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    trainer = NativeTrainer(_build('bilstm'), lr=1e-3)
    out = [_as_dict(trainer.predict(_dp_corpus(5), batch_size=2, threshold=0.5, return_tags=True, **kw)) for kw in DP_RUNS]
    out.append(_as_dict(trainer.predict(_dp_corpus(1), batch_size=2, threshold=0.5)))         # the second rank joins in without a document
    torch.save(out, os.path.join(out_dir, f'r{rank}.pt'))
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_return_the_single_process_prediction(tmp_path):
    import time
    import torch.multiprocessing as mp
    from multimodaltopicsegmentation_amd import predict
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
    model = _build('bilstm')
    alone = [_as_dict(predict(model, _dp_corpus(5), batch_size=2, threshold=0.5, return_tags=True, **kw)) for kw in DP_RUNS]
    alone.append(_as_dict(predict(model, _dp_corpus(1), batch_size=2, threshold=0.5)))
    for a, b, c in zip(r0, r1, alone):
        assert _same(a, b) and _same(a, c)
        assert a['documents'].tolist() == list(range(len(a['documents']))) and a['names'] == NAMES[:len(a['documents'])]
