"""GPU tests of the fit loop (fit.fit / NativeTrainer.fit) on tiny models and a resident corpus of 12 documents: the training path is the
hand-written loop bit for bit (with and without validation between the epochs), every epoch's threshold and table row are those of an
independent ThresholdSweep over the validation documents with that epoch's weights, the best state is restored, a one-rank process group
changes nothing, and the refusals."""
import os
import socket

import pytest
import torch

from tests.test_resident_corpus_cpu import _lines

pytestmark = pytest.mark.gpu
DEV = 'cuda'
TRAIN_LENGTHS = [40, 5, 17, 33, 6, 38, 26, 9, 12, 31, 22, 15]
VAL_LENGTHS = [21, 5, 40, 8, 13, 35, 7, 29, 10, 18, 6, 24]
KINDS = ['bilstm', 'transformer', 'latefusion']
BATCH, SEED = 4, 5


def _corpus(kind, lengths, seed):
    from multimodaltopicsegmentation_amd import AudioPortionDataset, ResidentCorpus
    d1, d2 = (40, 24) if kind == 'latefusion' else (64, None)
    second = _lines(lengths, D=d2, seed=seed + 1) if d2 else None
    return ResidentCorpus(AudioPortionDataset(_lines(lengths, D=d1, seed=seed, boundary_p=0.2), {}, CRF=False, truncate=False, second_input=second), DEV)


def _build(kind):
    from multimodaltopicsegmentation_amd import BiLSTM, BiLSTMLateFusion, Transformer_segmenter
    if kind == 'transformer':
        return Transformer_segmenter(2, 64, 32, num_layers=2, nheads=4, loss_fn='FocalLoss', window_size=4, compute_dtype='fp32',
                                     max_position_embedding=128, seed=11).to(DEV)
    if kind == 'bilstm':
        return BiLSTM(2, 64, 32, num_layers=2, loss_fn='FocalLoss', compute_dtype='fp32', seed=11).to(DEV)
    return BiLSTMLateFusion(2, [40, 24], 32, num_layers=2, loss_fn='FocalLoss', compute_dtype='fp32', seed=11).to(DEV)


def _hand_loop(kind, train, epochs, lr=1e-3):
    """sampler + corpus.batch + trainer.step, nothing else -> (model, per-epoch mean losses)"""
    from multimodaltopicsegmentation_amd.trainer import NativeTrainer
    model = _build(kind)
    tr = NativeTrainer(model, lr=lr)
    sampler = train.sampler(BATCH, rank=0, world=1, shuffle=True, seed=SEED)
    means = []
    for epoch in range(epochs):
        sampler.set_epoch(epoch)
        losses = [tr.step(train.batch(*item)) for item in sampler]
        means.append(float(torch.stack([v.detach() for v in losses]).to(torch.float64).sum()) / len(losses))
    return model, means


def _forward(model, batch):
    if batch.get('src_tokens2') is not None:
        return model(batch['src_tokens'], batch['src_tokens2'], batch['src_lengths'])[0]
    return model(batch['src_tokens'], batch['src_lengths'])[0]


def _loss(model, batch):
    with torch.no_grad():
        if batch.get('src_tokens2') is not None:
            return model.loss(batch['src_tokens'], batch['src_tokens2'], batch['src_lengths'], batch['tgt_tokens'])
        return model.loss(batch['src_tokens'], batch['src_lengths'], batch['tgt_tokens'])


def _twin(kind, flat):
    twin = _build(kind)
    with torch.no_grad():
        twin.flat.copy_(flat)
    return twin.eval()


@pytest.mark.parametrize('kind', KINDS)
def test_fit_is_the_hand_written_loop(kind):
    from multimodaltopicsegmentation_amd import fit
    from multimodaltopicsegmentation_amd.trainer import NativeTrainer
    train = _corpus(kind, TRAIN_LENGTHS, 2)
    want, means = _hand_loop(kind, train, 3)
    model = _build(kind)
    init = model.flat.detach().clone()
    seen = []
    out = NativeTrainer(model, lr=1e-3).fit(train, batch_size=BATCH, max_epochs=3, seed=SEED, on_epoch_end=seen.append)
    assert torch.equal(model.flat, want.flat) and float((model.flat - init).abs().max()) > 1e-3
    assert [r['train_loss'] for r in out['epochs']] == means == [r['monitored'] for r in out['epochs']]      # monitor = training_loss
    assert seen == out['epochs'] and [r['epoch'] for r in seen] == [0, 1, 2]
    assert all(r['lr'] == 1e-3 and r['threshold'] is None for r in seen) and out['threshold'] is None and not out['stopped_early']
    assert out['best_value'] == min(means) and out['best_epoch'] == means.index(min(means))
    # the module-level function is the method
    model2 = _build(kind)
    out2 = fit(NativeTrainer(model2, lr=1e-3), train, batch_size=BATCH, max_epochs=3, seed=SEED)
    assert out2 == out and torch.equal(model2.flat, model.flat)


@pytest.mark.parametrize('metric', ['Pk', 'F1', 'scaiano'])
@pytest.mark.parametrize('kind', KINDS)
def test_threshold_search_per_epoch_equals_an_independent_sweep(kind, metric):
    from multimodaltopicsegmentation_amd import ThresholdSweep
    from multimodaltopicsegmentation_amd.trainer import NativeTrainer
    train, val = _corpus(kind, TRAIN_LENGTHS, 2), _corpus(kind, VAL_LENGTHS, 6)
    model = _build(kind)
    flats = []
    tr = NativeTrainer(model, lr=1e-3)
    out = tr.fit(train, val, batch_size=BATCH, max_epochs=3, seed=SEED, search_threshold=True, metric=metric, restore_best=False,
                 on_epoch_end=lambda record: flats.append(model.flat.detach().clone()))
    # validation between the epochs leaves the training path alone
    assert torch.equal(model.flat, _hand_loop(kind, train, 3)[0].flat)
    assert len(flats) == 3 and torch.equal(flats[2], model.flat) and not torch.equal(flats[0], flats[1])
    for record, flat in zip(out['epochs'], flats):
        twin = _twin(kind, flat)
        sweep = ThresholdSweep(metric=metric)
        for s in range(0, len(val), BATCH):
            batch = val.batch(list(range(s, min(s + BATCH, len(val)))))
            sweep.add(_forward(twin, batch), batch['tgt_tokens'], batch['src_lengths'])
        assert sweep.counts().shape == (12, 19, 3 if metric == 'scaiano' else 6)
        row = sweep.best(metric)
        assert {k: record[k] for k in row} == row, (record, row)
        assert record['monitored'] == row['valid_loss'] and record['threshold'] == row['threshold']
        assert set(record) == set(row) | {'epoch', 'train_loss', 'monitored', 'lr'}
    best = (min if metric == 'Pk' else max)(r['monitored'] for r in out['epochs'])
    first = [r['monitored'] for r in out['epochs']].index(best)
    assert (out['best_epoch'], out['best_value'], out['threshold']) == (first, best, out['epochs'][first]['threshold'])
    assert model.th == out['epochs'][-1]['threshold']          # restore_best=False: the last epoch's threshold stays


def test_restore_best_and_the_validation_loss():
    """lr 0.3 makes the validation loss go up after some epoch (the premise of the early-stopping half: a run that ends on an epoch which is
    not its best, so that restoring is visible)."""
    from multimodaltopicsegmentation_amd.trainer import NativeTrainer
    kind = 'bilstm'
    train, val = _corpus(kind, TRAIN_LENGTHS, 2), _corpus(kind, VAL_LENGTHS, 6)
    model = _build(kind)
    model.th = None
    flats = []
    tr = NativeTrainer(model, lr=0.3)
    out = tr.fit(train, val, batch_size=BATCH, max_epochs=6, seed=SEED, lr_patience=0, lr_factor=0.5,
                 on_epoch_end=lambda record: flats.append(model.flat.detach().clone()))
    mon = [r['monitored'] for r in out['epochs']]
    for record, flat in zip(out['epochs'], flats):
        twin = _twin(kind, flat)
        total = docs = 0.0
        for s in range(0, len(val), BATCH):
            idx = list(range(s, min(s + BATCH, len(val))))
            total, docs = total + float(_loss(twin, val.batch(idx)).to(torch.float64)) * len(idx), docs + len(idx)
        assert abs(record['val_loss'] - total / docs) <= 1e-12 * abs(total / docs)      # float64 sums of three terms in two orders
        assert record['monitored'] == record['val_loss'] and record['threshold'] is None
    assert out['best_value'] == min(mon) and out['best_epoch'] == mon.index(min(mon)) and out['threshold'] is None
    assert torch.equal(model.flat, flats[out['best_epoch']]) and not torch.equal(flats[0], flats[-1])
    assert model.th is None
    # the schedule: torch's ReduceLROnPlateau(patience=0) on the same monitored values
    opt = torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=0.3)
    sched = torch.optim.lr_scheduler.ReduceLROnPlateau(opt, 'min', factor=0.5, patience=0)
    lrs = [0.3]
    for v in mon:
        sched.step(v)
        lrs.append(opt.param_groups[0]['lr'])
    assert [r['lr'] for r in out['epochs']] == lrs[:-1] and tr.lr == lrs[-1] and lrs[-1] < 0.3
    # early stopping on the same run: the first epoch that is not better than the best so far ends it
    model2 = _build(kind)
    out2 = NativeTrainer(model2, lr=0.3).fit(train, val, batch_size=BATCH, max_epochs=6, seed=SEED, lr_patience=0, lr_factor=0.5, patience=1)
    stop = next(e for e in range(1, 6) if mon[e] >= min(mon[:e]))
    assert out2['stopped_early'] and len(out2['epochs']) == stop + 1 and out2['epochs'] == out['epochs'][:stop + 1]
    assert out2['best_epoch'] < stop and not torch.equal(flats[out2['best_epoch']], flats[stop])      # the run ended on a worse epoch ...
    assert torch.equal(model2.flat, flats[out2['best_epoch']])                                        # ... and holds the best one's bits
    model3 = _build(kind)
    out3 = NativeTrainer(model3, lr=0.3).fit(train, val, batch_size=BATCH, max_epochs=6, seed=SEED, lr_patience=0, lr_factor=0.5, patience=1,
                                             restore_best=False)
    assert out3 == out2 and torch.equal(model3.flat, flats[stop])


def test_a_one_rank_process_group_changes_nothing():
    import torch.distributed as dist
    from multimodaltopicsegmentation_amd.trainer import NativeTrainer
    kind = 'bilstm'
    train, val = _corpus(kind, TRAIN_LENGTHS, 2), _corpus(kind, VAL_LENGTHS, 6)

    def run():
        model = _build(kind)
        out = NativeTrainer(model, lr=1e-3).fit(train, val, batch_size=BATCH, max_epochs=2, seed=SEED, search_threshold=True, metric='scaiano')
        return out, model.flat.detach().clone()
    alone, flat_alone = run()
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
    dist.init_process_group('gloo', rank=0, world_size=1)
    try:
        grouped, flat_grouped = run()
    finally:
        dist.destroy_process_group()
    assert grouped == alone and torch.equal(flat_grouped, flat_alone)


def test_refusals():
    from multimodaltopicsegmentation_amd import BiRnnCrf, fit
    from multimodaltopicsegmentation_amd.trainer import NativeTrainer
    train, val = _corpus('bilstm', TRAIN_LENGTHS, 2), _corpus('bilstm', VAL_LENGTHS, 6)
    crf = BiRnnCrf(2, 64, 32, num_layers=1, architecture='rnn', compute_dtype='fp32').to(DEV)
    before = crf.flat.detach().clone()
    with pytest.raises(NotImplementedError, match='biLSTMCRF'):
        fit(NativeTrainer(crf, lr=1e-3), train, val, batch_size=BATCH, max_epochs=1, search_threshold=True)
    assert torch.equal(crf.flat, before)                       # refused before the first step
    model = _build('bilstm')
    for metric in ('b', 'B'):
        with pytest.raises(NotImplementedError, match='segeval'):
            fit(NativeTrainer(model, lr=1e-3), train, val, batch_size=BATCH, max_epochs=1, search_threshold=True, metric=metric)
    with pytest.raises(ValueError):
        fit(NativeTrainer(model, lr=1e-3), train, batch_size=BATCH, max_epochs=1, search_threshold=True)


# ---- two ranks ----------------------------------------------------------------------------------------------------------------
DP_VAL = {'five': VAL_LENGTHS[:5], 'one': VAL_LENGTHS[:1]}      # 3 + 2 documents; 1 + 0: the second rank validates nothing and still joins in
DP_RUNS = [('five', True, 'scaiano'), ('five', False, 'Pk'), ('one', True, 'Pk')]


def _dp_worker(rank, world, port, out_dir):
    import torch.distributed as dist
    from multimodaltopicsegmentation_amd.trainer import NativeTrainer
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    torch.cuda.set_device(0)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    train = _corpus('bilstm', TRAIN_LENGTHS, 2)
    out = []
    for name, search, metric in DP_RUNS:
        val = _corpus('bilstm', DP_VAL[name], 6)
        model = _build('bilstm')
        flats = []
        rec = NativeTrainer(model, lr=1e-3).fit(train, val, batch_size=BATCH, max_epochs=2, seed=SEED, search_threshold=search, metric=metric,
                                                restore_best=False, on_epoch_end=lambda r: flats.append(model.flat.detach().cpu().clone()))
        out.append({'record': rec, 'flats': flats})
    torch.save(out, os.path.join(out_dir, f'r{rank}.pt'))
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_validate_their_own_documents_and_agree(tmp_path):
    import time
    import numpy as np
    import torch.multiprocessing as mp
    from multimodaltopicsegmentation_amd import ThresholdSweep
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
    for (name, search, metric), a, b in zip(DP_RUNS, r0, r1):
        assert a['record'] == b['record'], name                   # every rank returns the same values
        assert all(torch.equal(x, y) for x, y in zip(a['flats'], b['flats']))
        val = _corpus('bilstm', DP_VAL[name], 6)
        for record, flat in zip(a['record']['epochs'], a['flats']):
            twin = _twin('bilstm', flat.to(DEV))
            if search:
                # each rank's batches as the rank made them, the counts put into key order on the host: no gather() on this side
                counts, keys = [], []
                for rank in range(2):
                    docs = list(range(rank, len(val), 2))
                    for k in range(0, len(docs), BATCH):
                        batch = val.batch(docs[k:k + BATCH])
                        one = ThresholdSweep(metric=metric)
                        one.add(_forward(twin, batch), batch['tgt_tokens'], batch['src_lengths'])
                        counts.append(one.counts())
                        keys += docs[k:k + BATCH]
                merged = ThresholdSweep(metric=metric)
                merged.add_counts(np.concatenate(counts)[np.argsort(keys)])
                row = merged.best(metric)
                assert {k: record[k] for k in row} == row and record['monitored'] == row['valid_loss'], (name, record, row)
            else:
                total = 0.0
                for rank in range(2):
                    docs = list(range(rank, len(val), 2))
                    total += float(_loss(twin, val.batch(docs)).to(torch.float64)) * len(docs)
                assert abs(record['val_loss'] - total / len(val)) <= 1e-12 * abs(total / len(val))


def test_restore_best_refreshes_the_bf16_mirror():
    """bf16 compute: the optimizer kernel keeps a bf16 mirror of the fp32 master, so copying the best state back must make that mirror stale.
    lr 0.3 and patience 1 end the run on an epoch that is not its best (asserted: the premise)."""
    from multimodaltopicsegmentation_amd import Transformer_segmenter
    from multimodaltopicsegmentation_amd.trainer import NativeTrainer

    def build():
        return Transformer_segmenter(2, 64, 32, num_layers=2, nheads=4, loss_fn='FocalLoss', window_size=4, compute_dtype='bf16',
                                     max_position_embedding=128, seed=11).to(DEV)
    train, val = _corpus('transformer', TRAIN_LENGTHS, 2), _corpus('transformer', VAL_LENGTHS, 6)
    model = build()
    flats = []
    out = NativeTrainer(model, lr=0.3).fit(train, val, batch_size=BATCH, max_epochs=8, seed=SEED, patience=1,
                                           on_epoch_end=lambda record: flats.append(model.flat.detach().clone()))
    assert out['stopped_early'] and out['best_epoch'] < len(flats) - 1, [r['monitored'] for r in out['epochs']]
    assert torch.equal(model.flat, flats[out['best_epoch']]) and not torch.equal(model.flat, flats[-1])
    twin = build()
    with torch.no_grad():
        twin.flat.copy_(flats[out['best_epoch']])
    batch = val.batch([0, 1, 2, 3])
    assert torch.equal(_forward(model.eval(), batch), _forward(twin.eval(), batch))
    stale = build()
    with torch.no_grad():
        stale.flat.copy_(flats[-1])
    assert not torch.equal(_forward(stale.eval(), batch), _forward(twin.eval(), batch))        # a mirror of the last epoch would show
