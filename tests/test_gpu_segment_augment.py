"""Segment-order augmentation on the GPU: mts_gather_segments (csrc/gather.hip) against the host oracle's padded batch in every access width,
on both kernels, with segment edges in every phase of a wave's group of four rows and cuts inside and on the edge of a segment; the targets'
label rule; inputs the public ABI must survive (an index outside the corpus, a source range that leaves its document); ResidentCorpus.
batch_segments against ResidentCorpus.batch; AugmentedCorpus.batch in both modes; fit(augment=...) against the hand-written loop, on one rank
and on two.  Pure data movement: every comparison is torch.equal."""
import os
import time

import numpy as np
import pytest
import torch

from tests import segment_augment_oracle as O
from tests.test_segment_augment_cpu import LABELS, SEED, TV, _dataset

pytestmark = pytest.mark.gpu
DEV = 'cuda'
SENTINEL = 12288.0                               # exact in bf16 too; no input holds it
F32, BF16 = torch.float32, torch.bfloat16
ROWS = [len(y) for y in LABELS]                  # 1, 7, 5, 4, 37, 300
N = len(LABELS)

# (document, order, close_last) per batch row
IDENTITY = [(d, *O.identity_rule(LABELS[d])) for d in range(N)]
REVERSE = [(d, *O.reverse_rule(LABELS[d])) for d in range(N)]
# one fixed permutation, the full reverse with the tail and a single-segment subset of ONE document (three orders of it in one batch); a
# rotation; the 300-row document backwards (1 + 298 + 1 rows); five one-row segments backwards; the document without a boundary: 7 documents
MIXED = [(4, [3, 0, 5, 1, 4, 2], False), (4, [5, 4, 3, 2, 1, 0], False), (4, [4], True), (1, [1, 2, 0], False), (5, [2, 1, 0], False),
         (2, [4, 3, 2, 1, 0], False), (3, [0], False)]
BATCHES = {'identity': IDENTITY, 'reverse': REVERSE, 'mixed': MIXED}
# besides the exact fit and one row of pad: 5 (7 documents x 5 rows = 35 rows: a last, partial group of four); 6 and 23 (edges of the
# permuted document's segments 5 | 1 | 17 | 2 | 9 | 3), 20 (inside its 17-row segment), 299 (the edge behind the 298-row segment)
CUTS = [5, 6, 20, 23, 299]
_made = {}


def _row_start():
    return torch.tensor([0] + np.cumsum(ROWS).tolist(), dtype=torch.int64)


def _corpus(D, dtype):
    """host corpus of the six documents, made once per shape and left unchanged"""
    if (D, dtype) not in _made:
        c = torch.randn(sum(ROWS), D, generator=torch.Generator().manual_seed(D))
        _made[(D, dtype)] = c.to(dtype)
    return _made[(D, dtype)]


def _doc(corpus, d):
    s = int(np.cumsum([0] + ROWS)[d])
    return corpus[s:s + ROWS[d]]


def _tables(batch):
    """the listed-segment tables of a batch, built here from the labels alone (not by the product)"""
    idx, ptr, dst, src, length, close = [], [0], [], [], [], []
    for d, order, close_last in batch:
        seg = O.segment_ranges(LABELS[d])
        at = 0
        for j in order:
            dst.append(at)
            src.append(seg[j][0])
            at += seg[j][1] - seg[j][0]
        idx.append(d)
        ptr.append(len(dst))
        length.append(at)
        close.append(int(close_last))
    return [torch.tensor(v, dtype=torch.int32, device=DEV) for v in (idx, ptr, dst, src, length, close)]


def _gather(corpus_dev, tables, Lmax, pad, dst_dtype, labels=False):
    from multimodaltopicsegmentation_amd import ops
    idx, ptr, dst_off, src_off, length, close = tables
    dst = torch.full((idx.numel(), Lmax) + tuple(corpus_dev.shape[1:]), SENTINEL, dtype=dst_dtype, device=DEV)   # every element must be written
    ops.gather_segments(corpus_dev, _row_start().to(DEV), idx, ptr, dst_off, src_off, length, dst, pad, close_last=close if labels else None)
    return dst


def _lmaxes(batch):
    longest = max(sum(O.segment_ranges(LABELS[d])[j][1] - O.segment_ranges(LABELS[d])[j][0] for j in order) for d, order, _ in batch)
    return [longest, longest + 1] + CUTS


# D -> access (tests/test_gpu_resident_corpus.py): 64 = 16-byte units on the thin kernel; 520 (bf16) = 65 16-byte units and 1792 = configs[1] on
# the wave-per-row kernel; 770 fp32 -> bf16 = pairs in the cast; 771 = odd: 2-byte units; 6 = 12-byte bf16 rows
SHAPES = [(64, F32, F32), (64, BF16, BF16), (520, BF16, BF16), (1792, BF16, BF16), (770, F32, BF16), (771, BF16, BF16), (6, BF16, BF16)]


@pytest.mark.parametrize('D,src,dst', SHAPES, ids=lambda v: str(v).replace('torch.', ''))
def test_gather_segments_equals_the_oracles_padded_batch(D, src, dst):
    corpus = _corpus(D, src)
    dev = corpus.to(DEV)
    for name, batch in BATCHES.items():
        docs = [O.augment_document(_doc(corpus, d), LABELS[d], order, close)[0] for d, order, close in batch]
        tables = _tables(batch)
        for Lmax in _lmaxes(batch):
            got = _gather(dev, tables, Lmax, 0.0, dst).cpu()
            assert torch.equal(got, O.padded_batch(docs, Lmax, 0.0, dst)), (name, Lmax)


@pytest.mark.parametrize('pad', [-1.0, 0.0])
def test_targets_follow_the_label_rule(pad):
    """D = 1: gathered from the stored targets by the thin kernel, a 1 on the last row of every listed segment (the tail's too, where it is not
    the last) and close_last on the last row"""
    tg = torch.cat([torch.tensor(y, dtype=F32) for y in LABELS])
    dev = tg.to(DEV)
    for name, batch in BATCHES.items():
        labs = [O.augment_document(torch.zeros(ROWS[d], 1), LABELS[d], order, close)[1] for d, order, close in batch]
        tables = _tables(batch)
        for Lmax in _lmaxes(batch):
            got = _gather(dev, tables, Lmax, pad, F32, labels=True).cpu()
            assert got.shape == (len(batch), Lmax) and torch.equal(got.view(torch.int32), O.padded_batch(labs, Lmax, pad).view(torch.int32)), (name, Lmax)
    # without the rule the same entry point copies the stored labels: a plain reordering
    batch = MIXED
    plain = [O.augment_document(_doc(tg.view(-1, 1), d), LABELS[d], order, close)[0].view(-1) for d, order, close in batch]
    assert torch.equal(_gather(dev, _tables(batch), 300, pad, F32).cpu(), O.padded_batch(plain, 300, pad))


@pytest.mark.parametrize('D,src,dst', [(64, F32, F32), (1792, BF16, BF16), (770, F32, BF16), (1, F32, F32)], ids=lambda v: str(v).replace('torch.', ''))
def test_inputs_the_public_abi_takes_as_pad(D, src, dst):
    """A document index outside the corpus, a listed segment whose source range leaves its document on either side, a list that holds no row
    and list bounds outside the tables are ordinary inputs: pad rows and MTS_OK, no address formed from them."""
    from multimodaltopicsegmentation_amd import ops
    corpus = _corpus(D, src) if D > 1 else _corpus(1, F32).view(-1)
    dev = corpus.to(DEV)
    doc1 = _doc(corpus, 1)                                           # 7 rows; document 2's rows follow it in the corpus
    idx = [1, 6, 1, -1, 2147483647, 1, 1, -2147483648, 1, 1]
    #        b=0: rows 4.. of document 1 for 7 rows: 3 inside, 4 behind its end        b=2: from row -2: 2 in front of it, 5 inside
    #        b=5: first listed segment starts at destination row 2: rows 0, 1 held by none     b=6: an empty list     b=8, 9: list bounds outside
    ptr = [0, 1, 2, 3, 4, 5, 6, 6, 7, 900, 7]
    dst_off = [0, 0, 0, 0, 0, 2, 0]
    src_off = [4, 0, -2, 0, 0, 0, 0]
    length = [7] * 10
    Lmax = 9
    want = torch.full((10, Lmax) + tuple(corpus.shape[1:]), -1.0, dtype=corpus.dtype)
    want[0, :3] = doc1[4:7]
    want[2, 2:7] = doc1[0:5]
    want[5, 2:7] = doc1[0:5]
    dst_t = torch.full(want.shape, SENTINEL, dtype=dst, device=DEV)
    t = [torch.tensor(v, dtype=torch.int32, device=DEV) for v in (idx, ptr, dst_off, src_off, length)]
    ops.gather_segments(dev, _row_start().to(DEV), *t, dst_t, -1.0)     # check() raises on anything but MTS_OK
    torch.cuda.synchronize()
    assert torch.equal(dst_t.cpu(), want.to(dst))


def test_null_pointers_give_the_error_code():
    from multimodaltopicsegmentation_amd import _lib as L
    from multimodaltopicsegmentation_amd._lib import ptr
    corpus = _corpus(64, F32).to(DEV)
    tables = _tables(IDENTITY)
    dst = torch.full((N, 4, 64), SENTINEL, device=DEV)
    rs = _row_start().to(DEV)
    good = [ptr(corpus), ptr(rs), N, ptr(tables[0]), ptr(tables[1]), ptr(tables[2]), ptr(tables[3]), tables[2].numel(), ptr(tables[4]), None, ptr(dst)]
    for k in (0, 1, 3, 4, 5, 6, 8, 10):
        args = list(good)
        args[k] = None
        assert L.lib.mts_gather_segments(None, L.F32, L.F32, N, 4, 64, *args, 0.0) == 1, k
        assert b'mts_gather_segments' in L.lib.mts_last_error()
    with pytest.raises(ValueError):
        L.check(1)
    torch.cuda.synchronize()
    assert bool((dst == SENTINEL).all())                              # refused before any device work


# ---- ResidentCorpus.batch_segments and AugmentedCorpus.batch ------------------------------------------------------------------------

def _same_batch(got, ref):
    assert set(got) == set(ref)
    for f in ('src_tokens', 'src_tokens2', 'tgt_tokens'):
        if ref[f] is None:
            assert got[f] is None
            continue
        assert got[f].dtype == ref[f].dtype and got[f].device == ref[f].device and got[f].shape == ref[f].shape, f
        assert torch.equal(got[f].view(torch.int16 if got[f].dtype == BF16 else torch.int32), ref[f].view(torch.int16 if ref[f].dtype == BF16 else torch.int32)), f
    assert got['src_lengths'].dtype == ref['src_lengths'].dtype and torch.equal(got['src_lengths'], ref['src_lengths'])
    assert torch.equal(got['id'], ref['id']) and got['domain'] == ref['domain'] and got.get('src_segments') == ref.get('src_segments')


@pytest.mark.parametrize('truncate', [True, False])
@pytest.mark.parametrize('wire', ['fp32', 'bf16'])
def test_identity_orders_equal_the_plain_batch(wire, truncate):
    from multimodaltopicsegmentation_amd import ResidentCorpus
    rc = ResidentCorpus(_dataset(truncate, second=True, domain_adapt=True, segments=True), DEV, wire_dtype=wire)
    for idx in ([0, 1, 2, 3, 4, 5], [5, 5, 0, 2, 2], [4], [3, 0]):
        orders = [list(range(int(rc.n_segments[d]))) for d in idx]
        _same_batch(rc.batch_segments(idx, orders, False), rc.batch(idx))
    if not truncate:
        _same_batch(rc.batch_segments([1, 2], [[0, 1, 2], [0, 1, 2, 3, 4]], [False, False], pad_to=11), rc.batch([1, 2], pad_to=11))
    # the view's stored half is the plain batch, alone and next to twins
    view = rc.augmented('shuffle', seed=SEED)
    _same_batch(view.batch([2, 0, 5, 4]), rc.batch([2, 0, 5, 4]))
    mixed = view.batch([4, 10, 1])
    alone = rc.batch([4, 1], pad_to=None if truncate else mixed['src_tokens'].shape[1])
    assert torch.equal(mixed['src_tokens'][[0, 2]], alone['src_tokens']) and torch.equal(mixed['tgt_tokens'][[0, 2]], alone['tgt_tokens'])
    assert [mixed['src_segments'][0], mixed['src_segments'][2]] == alone['src_segments']


@pytest.mark.parametrize('truncate', [True, False])
@pytest.mark.parametrize('mode', ['reverse', 'shuffle'])
def test_augmented_batch_equals_the_oracle(mode, truncate):
    """truncate=True cuts at truncate_value = 6, below most augmented lengths; the second input is reordered with the first"""
    from multimodaltopicsegmentation_amd import ResidentCorpus
    ds = _dataset(truncate, second=True, domain_adapt=True, segments=True)
    rc = ResidentCorpus(ds, DEV, wire_dtype='bf16')
    view = rc.augmented(mode, seed=SEED)
    for epoch in (0, 3):
        view.set_epoch(epoch)
        for idx, pad_to in (([6, 7, 8, 9, 10, 11], None), ([10, 4, 1, 7, 10], None), ([11, 0], None), ([7, 8, 1], 12)):
            if truncate:
                pad_to = None
            docs, docs2, labs = [], [], []
            for v in idx:
                d = v % N
                y = LABELS[d]
                rule = O.identity_rule(y) if v < N else O.reverse_rule(y) if mode == 'reverse' else O.shuffle_rule(y, SEED, epoch, d)
                e, lab = O.augment_document(torch.as_tensor(ds.embeddings[d]), y, *rule)
                docs.append(e)
                docs2.append(O.augment_document(torch.as_tensor(ds.embeddings2[d]), y, *rule)[0])
                labs.append(lab)
            Lmax = TV if truncate else (pad_to or max(len(t) for t in labs))
            got = view.batch(idx, pad_to)
            assert torch.equal(got['src_tokens'].cpu(), O.padded_batch(docs, Lmax, 0.0, BF16)), (epoch, idx)
            assert torch.equal(got['src_tokens2'].cpu(), O.padded_batch(docs2, Lmax, 0.0, BF16)), (epoch, idx)
            assert torch.equal(got['tgt_tokens'].cpu(), O.padded_batch(labs, Lmax, -1.0)), (epoch, idx)
            lengths = [min(len(t), Lmax) if truncate else len(t) for t in labs]
            assert got['src_lengths'].tolist() == lengths and got['id'].tolist() == idx
            assert got['src_segments'] == [O.augmented_segments(t, n) for t, n in zip(labs, lengths)]
            assert got['domain'] == [rc.domain[v % N] for v in idx]
            host, Lh = view.host_fields(idx, pad_to)
            assert Lh == Lmax and host['src_segments'] == got['src_segments'] and torch.equal(host['src_lengths'], got['src_lengths'])


# ---- training ---------------------------------------------------------------------------------------------------------------------

TRAIN_LENGTHS = [40, 5, 17, 33, 6, 38, 26, 9, 12, 31, 22, 15]
BATCH, FIT_SEED, EPOCHS = 6, 5, 2


def _train_corpus():
    from multimodaltopicsegmentation_amd import AudioPortionDataset, ResidentCorpus
    from tests.test_resident_corpus_cpu import _lines
    return ResidentCorpus(AudioPortionDataset(_lines(TRAIN_LENGTHS, D=64, seed=2, boundary_p=0.2), {}, CRF=False, truncate=False), DEV)


def _build():
    from multimodaltopicsegmentation_amd import BiLSTM
    return BiLSTM(2, 64, 32, num_layers=2, loss_fn='FocalLoss', compute_dtype='fp32', seed=11).to(DEV)


@pytest.mark.parametrize('mode', ['shuffle', 'reverse'])
def test_fit_with_augment_is_the_hand_written_loop(mode):
    from multimodaltopicsegmentation_amd import fit
    from multimodaltopicsegmentation_amd.trainer import NativeTrainer
    train = _train_corpus()
    want = _build()
    tr = NativeTrainer(want, lr=1e-3)
    view = train.augmented(mode, seed=FIT_SEED)
    sampler = view.sampler(BATCH, rank=0, world=1, shuffle=True, seed=FIT_SEED)
    assert len(sampler) == 2 * len(TRAIN_LENGTHS) // BATCH
    means = []
    for epoch in range(EPOCHS):
        sampler.set_epoch(epoch)
        losses = []
        for item in sampler:
            losses.append(tr.step(view.batch(*item)))
        means.append(float(torch.stack([v.detach() for v in losses]).to(torch.float64).sum()) / len(losses))
    model = _build()
    init = model.flat.detach().clone()
    out = fit(NativeTrainer(model, lr=1e-3), train, batch_size=BATCH, max_epochs=EPOCHS, seed=FIT_SEED, augment=mode)
    assert torch.equal(model.flat, want.flat) and float((model.flat - init).abs().max()) > 1e-3
    assert [r['train_loss'] for r in out['epochs']] == means
    # the method passes the argument on, and without it nothing is augmented: another run
    model2, plain = _build(), _build()
    NativeTrainer(model2, lr=1e-3).fit(train, batch_size=BATCH, max_epochs=EPOCHS, seed=FIT_SEED, augment=mode)
    NativeTrainer(plain, lr=1e-3).fit(train, batch_size=BATCH, max_epochs=EPOCHS, seed=FIT_SEED)
    assert torch.equal(model2.flat, model.flat) and not torch.equal(plain.flat, model.flat)


def _dp_worker(rank, world, port, out_dir):
    import torch.distributed as dist
    from multimodaltopicsegmentation_amd.trainer import NativeTrainer
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    torch.cuda.set_device(0)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    train = _train_corpus()
    model = _build()
    record = NativeTrainer(model, lr=1e-3).fit(train, batch_size=BATCH, max_epochs=EPOCHS, seed=FIT_SEED, augment='shuffle')
    # this rank's share of every global batch, as the fit loop drew it
    view = train.augmented('shuffle', seed=FIT_SEED)
    sampler = view.sampler(BATCH, rank=rank, world=world, shuffle=True, seed=FIT_SEED)
    shares = []
    for epoch in range(EPOCHS):
        sampler.set_epoch(epoch)
        for item in sampler:
            b = view.batch(*item)
            shares.append({'id': b['id'], 'src_tokens': b['src_tokens'].cpu(), 'tgt_tokens': b['tgt_tokens'].cpu(), 'src_lengths': b['src_lengths']})
    torch.save({'record': record, 'flat': model.flat.detach().cpu(), 'shares': shares}, os.path.join(out_dir, f'r{rank}.pt'))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(600)
def test_two_ranks_draw_the_same_twins_and_end_alike(tmp_path):
    import torch.multiprocessing as mp
    from tests.test_gpu_dp_step import _free_port
    ctx = mp.spawn(_dp_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=False)
    deadline = time.monotonic() + 240
    try:
        while not ctx.join(timeout=5):                                # raises when a rank exits with a non-zero status
            assert time.monotonic() < deadline, 'the two ranks did not finish in 240 s'
    finally:
        for p in ctx.processes:
            if p.is_alive():
                p.kill()
    r0, r1 = (torch.load(os.path.join(tmp_path, f'r{r}.pt'), weights_only=False) for r in range(2))
    assert r0['record'] == r1['record'] and torch.equal(r0['flat'], r1['flat']) and len(r0['record']['epochs']) == EPOCHS
    # the two ranks' shares are the two shards of the one-rank run's batch, twins included
    view = _train_corpus().augmented('shuffle', seed=FIT_SEED)
    sampler = view.sampler(BATCH, rank=0, world=1, shuffle=True, seed=FIT_SEED)
    k = twins = 0
    for epoch in range(EPOCHS):
        sampler.set_epoch(epoch)
        for g, pad_to in sampler:
            whole = view.batch(g, pad_to)
            for r, share in enumerate((r0['shares'][k], r1['shares'][k])):
                assert share['id'].tolist() == g[r::2] and torch.equal(share['src_lengths'], whole['src_lengths'][r::2])
                assert torch.equal(share['src_tokens'], whole['src_tokens'][r::2].cpu()) and torch.equal(share['tgt_tokens'], whole['tgt_tokens'][r::2].cpu())
            twins += sum(v >= len(TRAIN_LENGTHS) for v in g)
            k += 1
    assert k == len(r0['shares']) == len(r1['shares']) and twins == EPOCHS * len(TRAIN_LENGTHS)
