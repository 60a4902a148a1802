"""Negative-sentence masking on the GPU: mts_mask_plan (csrc/mask_plan.hip) against the host oracle at document lengths around a wave, around
the workgroup's rows per chunk and beyond two chunks, with cuts on and off a kept count; mts_gather_rows (csrc/gather.hip) against the
oracle's padded batch in every access width, on both kernels, with table edges in every phase of a wave's group of four rows and entries
the public ABI must take as pad; ResidentCorpus.batch_masked / MaskedCorpus.batch against the oracle; fit(mask_inner=...) against the
hand-written loop, on one rank and on two.  Integers and data movement: every comparison is torch.equal."""
import os
import time

import numpy as np
import pytest
import torch

from tests import mask_oracle as O
from tests.segment_augment_oracle import padded_batch
from tests.test_mask_inner_cpu import LABELS, N, SEED
from tests.test_segment_augment_cpu import TV, _dataset

pytestmark = pytest.mark.gpu
DEV = 'cuda'
SENTINEL = 12288.0                               # exact in bf16 too; no input holds it
UNWRITTEN = -7                                   # prefill of the plan's outputs: neither a row nor -1
F32, BF16 = torch.float32, torch.bfloat16
MASK_CHUNK = 256                                 # rows the plan kernel's workgroup takes per trip (csrc/mask_plan.hip), as built

# ---- mts_mask_plan ------------------------------------------------------------------------------------------------------------------
# a row, two, around a wave, around a chunk, more than two chunks, the inference config's 2 437 rows; all boundaries; no boundary (more than
# a wave, so that whole waves vote 0); a document without rows
PLAN_ROWS = [1, 2, 63, 64, 65, MASK_CHUNK - 1, MASK_CHUNK, MASK_CHUNK + 1, 2 * MASK_CHUNK + 188, 2437, 70, 130, 0]
ALL_POSITIVE, ALL_NEGATIVE, NO_ROWS = 10, 11, 12
_plan = {}


def _plan_corpus():
    """labels of the plan's documents (boundary share 0.1), their row table and the batch: every document, the 2 437-row one a second time
    under another seed, and three indices outside the corpus; made once and left unchanged"""
    if not _plan:
        g = np.random.default_rng(7)
        labels = [(g.random(n) < 0.1).astype(np.float32) for n in PLAN_ROWS]
        labels[ALL_POSITIVE][:] = 1.0
        labels[ALL_NEGATIVE][:] = 0.0
        idx = list(range(len(PLAN_ROWS))) + [9, -1, len(PLAN_ROWS), 2147483647]
        seeds = [O.doc_seed(5, 1, len(PLAN_ROWS), d % len(PLAN_ROWS)) for d in idx]
        seeds[len(PLAN_ROWS)] = 2 ** 64 - 3                                       # the repeat: another seed, with the top bit set
        _plan.update(labels=labels, idx=idx, seeds=seeds, start=np.concatenate([[0], np.cumsum(PLAN_ROWS)]).astype(np.int64))
    return _plan


def _seed_tensor(seeds):
    return torch.from_numpy(np.array(seeds, dtype=np.uint64).view(np.int64).copy()).to(DEV)


@pytest.mark.parametrize('p', [0.0, 0.5, 1.0])
def test_mask_plan_equals_the_oracle(p):
    from multimodaltopicsegmentation_amd import ops
    c = _plan_corpus()
    n_docs = len(PLAN_ROWS)
    kept_rows = [O.kept_rows(c['labels'][d].tolist(), s, p) if 0 <= d < n_docs else [] for d, s in zip(c['idx'], c['seeds'])]
    counts = [len(k) for k in kept_rows]
    assert counts[NO_ROWS] == 0 and counts[-3:] == [0, 0, 0] and counts[ALL_POSITIVE] == 70
    assert counts[ALL_NEGATIVE] == {0.0: 1, 1.0: 130}.get(p, counts[ALL_NEGATIVE])
    if p == 0.5:
        assert kept_rows[9] != kept_rows[n_docs] and 0 < counts[ALL_NEGATIVE] < 130      # two seeds, two draws of one document
    longest = max(counts)
    tg = torch.from_numpy(np.concatenate(c['labels'])).to(DEV)
    rs = torch.from_numpy(c['start']).to(DEV)
    idx = torch.tensor(c['idx'], dtype=torch.int32, device=DEV)
    seeds = _seed_tensor(c['seeds'])
    # the exact fit, a column of -1 behind it, one row, a cut ON the 65-row document's kept count (and so inside the longer ones), one
    # inside most documents, one behind a chunk
    for Lmax in sorted({longest, longest + 1, 1, counts[4], 37, MASK_CHUNK + 3}):
        src_row = torch.full((len(c['idx']), Lmax), UNWRITTEN, dtype=torch.int32, device=DEV)
        kept = torch.full((len(c['idx']),), UNWRITTEN, dtype=torch.int32, device=DEV)
        ops.mask_plan(tg, rs, idx, seeds, p, src_row, kept)
        want = [(k + [-1] * Lmax)[:Lmax] for k in kept_rows]
        assert kept.cpu().tolist() == counts, Lmax                      # not clipped to Lmax
        assert torch.equal(src_row.cpu(), torch.tensor(want, dtype=torch.int32)), Lmax


# ---- mts_gather_rows ----------------------------------------------------------------------------------------------------------------
ROWS = [len(y) for y in LABELS]                  # 1, 7, 5, 4, 37, 300, 5, 7
_made = {}


def _row_start():
    return torch.tensor([0] + np.cumsum(ROWS).tolist(), dtype=torch.int64)


def _corpus(D, dtype):
    """host corpus of the eight documents ([total_rows, D], or [total_rows] for D = 0: their labels), made once per shape and left unchanged"""
    if (D, dtype) not in _made:
        if D == 0:
            _made[(D, dtype)] = torch.cat([torch.tensor(y, dtype=F32) for y in LABELS])
        else:
            _made[(D, dtype)] = torch.randn(sum(ROWS), D, generator=torch.Generator().manual_seed(D)).to(dtype)
    return _made[(D, dtype)]


def _tables():
    """name -> (doc_index, src_row as B lists of Lmax entries).  The masked plans come from the oracle, not from the device."""
    if 'tables' in _made:
        return _made['tables']
    out = {}
    idx = list(range(N)) + [5]
    kept = [O.kept_rows(LABELS[d], O.doc_seed(SEED, k, N, d), 0.5) for k, d in enumerate(idx)]
    longest = max(len(k) for k in kept)
    # 9 batch rows: Lmax = longest + 1 and 6 give a row count that is no multiple of four (a last, partial group); 21 cuts the long ones
    for Lmax in (longest, longest + 1, 21, 6):
        out[f'masked{Lmax}'] = (idx, [(k + [-1] * Lmax)[:Lmax] for k in kept])
    out['identity'] = (list(range(N)), [list(range(n)) + [-1] * (300 - n) for n in ROWS])
    # any order, repeats, entries that are negative or at / behind the document's end (pad, no address formed), an index outside the corpus
    out['hand'] = ([1, 5, 4, N, -1, 2, 1],
                   [[6, 5, 4, 3, 2, 1, 0, 0, 7], [299, 300, 0, -1, 150, 150, 2147483647, -2147483648, 298], [36, 37, -5, 0, 1, 2, 3, 4, 5],
                    [0, 1, 2, 3, 4, 5, 6, 7, 8], [0, 0, 0, 0, 0, 0, 0, 0, 0], [5, 4, 4, 0, -1, -1, 1, 2, 3], [-1, -1, -1, 7, 8, 6, -1, 0, 1]])
    # the tables' edges (a valid entry next to a pad one, either way round) fall in every phase of a wave's group of four destination rows
    phases = set()
    for _, rows in out.values():
        flat = [e for r in rows for e in r]
        phases |= {t % 4 for t in range(1, len(flat)) if (flat[t] < 0) != (flat[t - 1] < 0)}
    assert phases == {0, 1, 2, 3}
    _made['tables'] = out
    return out


def _gather(corpus_dev, idx, rows, pad, dst_dtype):
    from multimodaltopicsegmentation_amd import ops
    table = torch.tensor(rows, dtype=torch.int32, device=DEV)
    dst = torch.full(tuple(table.shape) + tuple(corpus_dev.shape[1:]), SENTINEL, dtype=dst_dtype, device=DEV)      # every element must be written
    return ops.gather_rows(corpus_dev, _row_start().to(DEV), torch.tensor(idx, dtype=torch.int32, device=DEV), table, dst, pad)


# D -> access (tests/test_gpu_resident_corpus.py): 64 = 16-byte units on the thin kernel; 520 (bf16) = 65 16-byte units and 1792 = configs[1] on
# the wave-per-row kernel; 770 fp32 -> bf16 = pairs in the cast; 771 = odd: 2-byte units; 6 = 12-byte bf16 rows
SHAPES = [(64, F32, F32), (64, BF16, BF16), (520, BF16, BF16), (1792, BF16, BF16), (770, F32, BF16), (771, BF16, BF16), (6, BF16, BF16)]


@pytest.mark.parametrize('D,src,dst', SHAPES, ids=lambda v: str(v).replace('torch.', ''))
def test_gather_rows_equals_the_oracles_padded_batch(D, src, dst):
    from multimodaltopicsegmentation_amd import ops
    corpus = _corpus(D, src)
    dev = corpus.to(DEV)
    rs = _row_start()
    for name, (idx, rows) in _tables().items():
        got = _gather(dev, idx, rows, 0.0, dst)
        assert torch.equal(got.cpu(), O.gather_rows(corpus, rs.tolist(), idx, rows, 0.0, dst)), name
        if name == 'identity':                                          # every row in place: mts_gather_pad, bit for bit
            plain = torch.full(got.shape, SENTINEL, dtype=dst, device=DEV)
            ops.gather_pad(dev, rs.to(DEV), torch.tensor(idx, dtype=torch.int32, device=DEV), plain, 0.0)
            assert torch.equal(got.view(torch.int16 if dst == BF16 else torch.int32), plain.view(torch.int16 if dst == BF16 else torch.int32))


@pytest.mark.parametrize('pad', [-1.0, 0.0])
def test_targets_travel_with_their_rows(pad):
    """D = 1 on the thin kernel: the stored labels of the table's rows, not rewritten"""
    tg = _corpus(0, F32)
    dev = tg.to(DEV)
    for name, (idx, rows) in _tables().items():
        got = _gather(dev, idx, rows, pad, F32).cpu()
        assert got.shape == (len(idx), len(rows[0])), name
        assert torch.equal(got.view(torch.int32), O.gather_rows(tg, _row_start().tolist(), idx, rows, pad).view(torch.int32)), name


def test_null_pointers_give_the_error_code():
    from multimodaltopicsegmentation_amd import _lib as L
    from multimodaltopicsegmentation_amd._lib import ptr
    corpus = _corpus(64, F32).to(DEV)
    rs = _row_start().to(DEV)
    idx = torch.arange(N, dtype=torch.int32, device=DEV)
    table = torch.zeros((N, 4), dtype=torch.int32, device=DEV)
    dst = torch.full((N, 4, 64), SENTINEL, device=DEV)
    good = [ptr(corpus), ptr(rs), N, ptr(idx), ptr(table), ptr(dst)]
    for k in (0, 1, 3, 4, 5):
        args = list(good)
        args[k] = None
        assert L.lib.mts_gather_rows(None, L.F32, L.F32, N, 4, 64, *args, 0.0) == 1, k
        assert b'mts_gather_rows' in L.lib.mts_last_error()
    tg = _corpus(0, F32).to(DEV)
    seeds = _seed_tensor([1] * N)
    kept = torch.full((N,), UNWRITTEN, dtype=torch.int32, device=DEV)
    table.fill_(UNWRITTEN)
    good = [ptr(tg), ptr(rs), N, ptr(idx), ptr(seeds), 0.5, ptr(table), ptr(kept)]
    for k in (0, 1, 3, 4, 6, 7):
        args = list(good)
        args[k] = None
        assert L.lib.mts_mask_plan(None, N, 4, *args) == 1, k
        assert b'mts_mask_plan' in L.lib.mts_last_error()
    torch.cuda.synchronize()
    assert bool((dst == SENTINEL).all()) and bool((table == UNWRITTEN).all()) and bool((kept == UNWRITTEN).all())      # refused before any device work


# ---- ResidentCorpus.batch_masked and MaskedCorpus.batch ------------------------------------------------------------------------------

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
@pytest.mark.parametrize('second', [False, True], ids=['early', 'late'])
def test_probability_one_equals_the_plain_batch(second, wire, truncate):
    from multimodaltopicsegmentation_amd import ResidentCorpus
    rc = ResidentCorpus(_dataset(truncate, second=second, domain_adapt=True, segments=True, labels=LABELS), DEV, wire_dtype=wire)
    view = rc.masked(1.0, seed=SEED)
    for idx in (list(range(N)), [5, 5, 0, 2, 2], [4], [3, 0]):
        _same_batch(view.batch(idx), rc.batch(idx))
        _same_batch(rc.batch_masked(idx, [3] * len(idx), 1.0), rc.batch(idx))        # the low-level call, lengths from its own host pass
    if not truncate:
        _same_batch(view.batch([1, 2], pad_to=11), rc.batch([1, 2], pad_to=11))


@pytest.mark.parametrize('truncate', [True, False])
@pytest.mark.parametrize('p', [0.0, 0.25, 0.5, 0.9])
def test_masked_batch_equals_the_oracle(p, truncate):
    """late fusion in bf16 with segments and domains; truncate=True cuts at truncate_value = 6, below most masked lengths.  The second input
    and the labels travel with the first input's rows; the device's kept counts equal the host plan's and src_lengths is their cut."""
    from multimodaltopicsegmentation_amd import ResidentCorpus
    ds = _dataset(truncate, second=True, domain_adapt=True, segments=True, labels=LABELS)
    rc = ResidentCorpus(ds, DEV, wire_dtype='bf16')
    view = rc.masked(p, seed=SEED)
    for epoch in (0, 3):
        view.set_epoch(epoch)
        for idx, extra in ((list(range(N)), 0), ([5, 4, 1, 7, 5], 0), ([6, 0], 0), ([7, 6, 1], 5)):
            seeds = [O.doc_seed(SEED, epoch, N, d) for d in idx]
            masked = [O.mask_document(torch.as_tensor(ds.embeddings[d]), LABELS[d], s, p) for d, s in zip(idx, seeds)]
            docs2 = [O.mask_document(torch.as_tensor(ds.embeddings2[d]), LABELS[d], s, p)[0] for d, s in zip(idx, seeds)]
            counts = [len(lab) for _, lab in masked]
            pad_to = None if truncate or not extra else max(counts) + extra
            Lmax = TV if truncate else (pad_to or max(counts))
            lengths = [min(n, TV) if truncate else n for n in counts]
            got = view.batch(idx, pad_to)
            assert torch.equal(got['src_tokens'].cpu(), padded_batch([e for e, _ in masked], Lmax, 0.0, BF16)), (epoch, idx)
            assert torch.equal(got['src_tokens2'].cpu(), padded_batch(docs2, Lmax, 0.0, BF16)), (epoch, idx)
            assert torch.equal(got['tgt_tokens'].cpu(), padded_batch([lab for _, lab in masked], Lmax, -1.0)), (epoch, idx)
            assert got['src_lengths'].tolist() == lengths and got['id'].tolist() == idx and got['src_lengths'].dtype == torch.int64
            assert got['src_segments'] == [O.segments(lab, n) for (_, lab), n in zip(masked, lengths)]
            assert got['domain'] == [rc.domain[d] for d in idx]
            host, Lh = view.host_fields(idx, pad_to)
            assert Lh == Lmax and host['src_segments'] == got['src_segments'] and torch.equal(host['src_lengths'], got['src_lengths'])
            # the low-level call with the same seeds, and the device's own plan next to it
            low, src_row, kept = rc.batch_masked(idx, seeds, p, pad_to=pad_to, return_plan=True)
            _same_batch(low, got)
            assert kept.dtype == torch.int32 and kept.cpu().tolist() == counts == [int(view.rows[d]) for d in idx]
            assert [min(n, TV) if truncate else n for n in kept.cpu().tolist()] == got['src_lengths'].tolist()
            assert src_row.cpu().tolist() == [O.plan(LABELS[d], s, p, Lmax)[0] for d, s in zip(idx, seeds)]
            assert [src_row[k, :min(n, Lmax)].cpu().tolist() for k, n in enumerate(counts)] == [view.kept_rows(d)[:Lmax].tolist() for d in idx]


def test_early_fusion_fp32_without_segments():
    from multimodaltopicsegmentation_amd import ResidentCorpus
    ds = _dataset(False, labels=LABELS)
    rc = ResidentCorpus(ds, DEV)
    view = rc.masked(0.5, seed=SEED)
    idx = [7, 5, 6, 0]
    got = view.batch(idx)
    masked = [O.mask_document(torch.as_tensor(ds.embeddings[d]), LABELS[d], O.doc_seed(SEED, 0, N, d), 0.5) for d in idx]
    Lmax = max(len(lab) for _, lab in masked)
    assert got['src_tokens2'] is None and 'src_segments' not in got and got['domain'] is None and got['src_tokens'].dtype == F32
    assert torch.equal(got['src_tokens'].cpu(), padded_batch([e for e, _ in masked], Lmax, 0.0))
    assert torch.equal(got['tgt_tokens'].cpu(), padded_batch([lab for _, lab in masked], Lmax, -1.0))
    assert got['src_lengths'].tolist() == [len(lab) for _, lab in masked]


# ---- training ---------------------------------------------------------------------------------------------------------------------

TRAIN_LENGTHS = [40, 5, 17, 33, 6, 38, 26, 9, 12, 31, 22, 15]
BATCH, FIT_SEED, EPOCHS, KEEP = 6, 5, 2, 0.5


def _train_corpus():
    from multimodaltopicsegmentation_amd import AudioPortionDataset, ResidentCorpus
    from tests.test_resident_corpus_cpu import _lines
    return ResidentCorpus(AudioPortionDataset(_lines(TRAIN_LENGTHS, D=64, seed=2, boundary_p=0.2), {}, CRF=False, truncate=False), DEV)


def _build():
    from multimodaltopicsegmentation_amd import BiLSTM
    return BiLSTM(2, 64, 32, num_layers=2, loss_fn='FocalLoss', compute_dtype='fp32', seed=11).to(DEV)


def test_fit_with_mask_inner_is_the_hand_written_loop():
    from multimodaltopicsegmentation_amd import fit
    from multimodaltopicsegmentation_amd.trainer import NativeTrainer
    train = _train_corpus()
    want = _build()
    tr = NativeTrainer(want, lr=1e-3)
    view = train.masked(KEEP, seed=FIT_SEED)
    sampler = view.sampler(BATCH, rank=0, world=1, shuffle=True, seed=FIT_SEED)
    assert len(sampler) == len(TRAIN_LENGTHS) // BATCH
    means, shorter = [], 0
    for epoch in range(EPOCHS):
        sampler.set_epoch(epoch)
        losses = []
        for item in sampler:
            batch = view.batch(*item)
            shorter += int((batch['src_lengths'] < torch.from_numpy(train.lengths[item[0]])).sum())
            losses.append(tr.step(batch))
        means.append(float(torch.stack([v.detach() for v in losses]).to(torch.float64).sum()) / len(losses))
    assert shorter > EPOCHS * len(TRAIN_LENGTHS) // 2                    # most documents lost sentences
    model = _build()
    init = model.flat.detach().clone()
    out = fit(NativeTrainer(model, lr=1e-3), train, batch_size=BATCH, max_epochs=EPOCHS, seed=FIT_SEED, mask_inner=KEEP)
    assert torch.equal(model.flat, want.flat) and float((model.flat - init).abs().max()) > 1e-3
    assert [r['train_loss'] for r in out['epochs']] == means
    # the method passes the argument on, and without it nothing is masked: another run
    model2, plain = _build(), _build()
    NativeTrainer(model2, lr=1e-3).fit(train, batch_size=BATCH, max_epochs=EPOCHS, seed=FIT_SEED, mask_inner=KEEP)
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
    record = NativeTrainer(model, lr=1e-3).fit(train, batch_size=BATCH, max_epochs=EPOCHS, seed=FIT_SEED, mask_inner=KEEP)
    # the hand-written loop on this rank, on a second model: its share of every global batch, as the fit loop drew it
    by_hand = _build()
    tr = NativeTrainer(by_hand, lr=1e-3)
    view = train.masked(KEEP, seed=FIT_SEED)
    sampler = view.sampler(BATCH, rank=rank, world=world, shuffle=True, seed=FIT_SEED)
    shares, sums = [], []
    for epoch in range(EPOCHS):
        sampler.set_epoch(epoch)
        losses = []
        for item in sampler:
            b = view.batch(*item)
            shares.append({'id': b['id'], 'src_tokens': b['src_tokens'].cpu(), 'tgt_tokens': b['tgt_tokens'].cpu(), 'src_lengths': b['src_lengths']})
            losses.append(tr.step(b))
        sums.append((float(torch.stack([v.detach() for v in losses]).to(torch.float64).sum()), len(losses)))
    torch.save({'record': record, 'flat': model.flat.detach().cpu(), 'shares': shares, 'hand_flat': by_hand.flat.detach().cpu(), 'hand_sums': sums},
               os.path.join(out_dir, f'r{rank}.pt'))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(600)
def test_two_ranks_draw_the_same_masks_and_end_alike(tmp_path):
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
    # the two ranks' shares are the two shards of the one-rank run's masked batch
    view = _train_corpus().masked(KEEP, seed=FIT_SEED)
    sampler = view.sampler(BATCH, rank=0, world=1, shuffle=True, seed=FIT_SEED)
    k = 0
    for epoch in range(EPOCHS):
        sampler.set_epoch(epoch)
        for g, pad_to in sampler:
            whole = view.batch(g, pad_to)
            for r, share in enumerate((r0['shares'][k], r1['shares'][k])):
                assert share['id'].tolist() == g[r::2] and torch.equal(share['src_lengths'], whole['src_lengths'][r::2])
                assert torch.equal(share['src_tokens'], whole['src_tokens'][r::2].cpu()) and torch.equal(share['tgt_tokens'], whole['tgt_tokens'][r::2].cpu())
            k += 1
    assert k == len(r0['shares']) == len(r1['shares']) == EPOCHS * (len(TRAIN_LENGTHS) // BATCH)
    # fit on two ranks IS the hand-written two-rank loop over the view: final parameters and the epochs' mean losses, bit for bit
    assert torch.equal(r0['hand_flat'], r0['flat']) and torch.equal(r1['hand_flat'], r1['flat'])
    means = [(a[0] + b[0]) / (a[1] + b[1]) for a, b in zip(r0['hand_sums'], r1['hand_sums'])]
    assert [r['train_loss'] for r in r0['record']['epochs']] == means
