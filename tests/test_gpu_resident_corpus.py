"""The device-resident corpus on the GPU: mts_gather_pad (csrc/gather.hip) against a padded batch built on the host, in every access
width and on both kernels (rows of 64 or more units: one wave per row; thinner rows: one lane per unit); 64-bit offsets;
ResidentCorpus.batch against the reference collater; a training step from a resident batch; two data-parallel ranks that each gather
only their own documents."""
import os
import time

import pytest
import torch

from tests.test_resident_corpus_cpu import CASES, LENGTHS, _dataset, _lines

pytestmark = pytest.mark.gpu
DEV = 'cuda'
DOC_ROWS = [1, 7, 300, 64]
LMAXES = [5, 64, 300, 301]                       # truncation, an exact fit of the 64- and the 300-row document, trailing pad
SENTINEL = 12288.0                               # exact in bf16 too
_corpora = {}


def _corpus(D, dtype, special=False):
    """host corpus of DOC_ROWS documents, made once per shape and left unchanged"""
    key = (D, dtype, special)
    if key not in _corpora:
        g = torch.Generator().manual_seed(D)
        c = torch.randn(sum(DOC_ROWS), D, generator=g)
        if special:
            # NaN, +-Inf, ties to even (down to 1.0, up to 1.015625), a carry into the next exponent (-> 2.0), the largest float (-> Inf),
            # signed zero, a subnormal
            vals = torch.tensor([float('nan'), float('inf'), -float('inf'), 1.00390625, 1.01171875, 1.998046875, 1.9990234375,
                                 3.4028234663852886e38, -3.4028234663852886e38, -0.0, 1e-40, -1.00390625])
            flat = c.view(-1)
            pos = torch.randperm(flat.numel(), generator=g)[:vals.numel() * 40]
            flat[pos] = vals.repeat(40)
            flat[:vals.numel()] = vals                           # the length-1 document holds them too
        _corpora[key] = c.to(dtype)
    return _corpora[key]


def _row_start(rows=DOC_ROWS):
    return torch.tensor([0] + torch.tensor(rows).cumsum(0).tolist(), dtype=torch.int64)


def _host_batch(corpus, rows, idx, Lmax, pad, dst_dtype):
    start = _row_start(rows).tolist()
    out = torch.full((len(idx), Lmax) + tuple(corpus.shape[1:]), pad, dtype=corpus.dtype)
    for b, d in enumerate(idx):
        if 0 <= d < len(rows):
            n = min(rows[d], Lmax)
            out[b, :n] = corpus[start[d]:start[d] + n]
    return out.to(dst_dtype)


def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _gather(corpus_dev, idx, Lmax, pad, dst_dtype, rows=DOC_ROWS):
    from multimodaltopicsegmentation_amd import ops
    shape = (len(idx), Lmax) + tuple(corpus_dev.shape[1:])
    dst = torch.full(shape, SENTINEL, dtype=dst_dtype, device=DEV)          # a sentinel no input holds: every element must be written
    ops.gather_pad(corpus_dev, _row_start(rows).to(DEV), torch.tensor(idx, dtype=torch.int32, device=DEV), dst, pad)
    return dst


F32, BF16 = torch.float32, torch.bfloat16
# D -> access: 64 = 16-byte units on the thin kernel; 512 / 520 (bf16) = 64 / 65 16-byte units: the wave-per-row kernel's first sizes;
# 1792 = BASELINE configs[1]; 770 = rows that are no multiple of 16 bytes (8-byte units in fp32, 4-byte in bf16, pairs in the cast);
# 771 = odd: 2-byte units in bf16, single elements in the cast; 6 = 12-byte bf16 rows
SHAPES = [(64, F32, F32), (64, BF16, BF16), (64, F32, BF16), (512, BF16, BF16), (520, BF16, BF16), (1792, BF16, BF16), (1792, F32, F32),
          (1792, F32, BF16), (770, F32, F32), (770, BF16, BF16), (770, F32, BF16), (771, BF16, BF16), (771, F32, BF16), (6, BF16, BF16)]


@pytest.mark.parametrize('D,src,dst', SHAPES, ids=lambda v: str(v).replace('torch.', ''))
def test_gather_equals_the_host_batch(D, src, dst):
    corpus = _corpus(D, src)
    dev = corpus.to(DEV)
    idx = [2, 0, 3, 1, 2, 2, 0]                                  # repeats; 7 documents x Lmax 5 = 35 rows: a last, partial group of rows
    for Lmax in LMAXES:
        got = _gather(dev, idx, Lmax, 0.0, dst)
        assert torch.equal(got.cpu(), _host_batch(corpus, DOC_ROWS, idx, Lmax, 0.0, dst)), Lmax
    assert torch.equal(_gather(dev, [3], 64, 0.0, dst).cpu(), _host_batch(corpus, DOC_ROWS, [3], 64, 0.0, dst))          # B = 1
    assert torch.equal(_gather(dev, [0], 301, -1.0, dst).cpu(), _host_batch(corpus, DOC_ROWS, [0], 301, -1.0, dst))


@pytest.mark.parametrize('D,src,dst', [(64, F32, F32), (1792, BF16, BF16), (770, F32, BF16), (1, F32, F32)], ids=lambda v: str(v).replace('torch.', ''))
def test_an_index_outside_the_corpus_gives_an_all_pad_document(D, src, dst):
    corpus = _corpus(D, src)
    idx = [1, 4, 2, -1, 2147483647, -2147483648, 3]
    for pad in (0.0, -1.0):
        got = _gather(corpus.to(DEV), idx, 64, pad, dst).cpu()
        assert torch.equal(got, _host_batch(corpus, DOC_ROWS, idx, 64, pad, dst))
        for b in (1, 3, 4, 5):
            assert bool((got[b] == pad).all())


@pytest.mark.parametrize('pad', [-1.0, 0.0])
def test_targets_take_the_same_entry_point(pad):
    tg = (_corpus(1, F32) > 0.5).float().view(-1)                 # [total_rows]: D = 1
    idx = [2, 0, 3, 1, 2]
    for Lmax in LMAXES:
        got = _gather(tg.to(DEV), idx, Lmax, pad, F32)
        assert got.shape == (5, Lmax) and torch.equal(_bits(got.cpu()), _bits(_host_batch(tg, DOC_ROWS, idx, Lmax, pad, F32))), Lmax


@pytest.mark.parametrize('D', [64, 770, 771, 1024])
def test_narrowing_gives_torchs_bfloat16_bits(D):
    """Every element has the bits of torch's ``.to(torch.bfloat16)``: the device conversion's everywhere, the host conversion's at every
    element that is not a NaN.  The host conversion has no single answer for a NaN: the CPU build's vector loop writes 0xFFFF and its
    scalar tail 0x7FC0 for the same 0x7FC00000, depending on where in the tensor the element sits (seen on the MI355X host: element 0 of
    a [4, 5, 64] batch came out as 0xFFFF).  There the kernel must give a quiet NaN, which is what 'keeps NaN quiet' asks."""
    corpus = _corpus(D, F32, special=True)
    assert bool(corpus.isnan().any()) and bool(corpus.isinf().any())
    idx = [0, 2, 3, 1]
    for Lmax in (5, 301):
        got = _gather(corpus.to(DEV), idx, Lmax, 0.0, BF16).cpu()
        ref32 = _host_batch(corpus, DOC_ROWS, idx, Lmax, 0.0, F32)
        assert torch.equal(_bits(got), _bits(ref32.to(DEV).to(torch.bfloat16).cpu()))
        host, nan = ref32.to(torch.bfloat16), ref32.isnan()
        assert bool(nan.any()) and torch.equal(_bits(got)[~nan], _bits(host)[~nan])
        assert bool(host[nan].isnan().all()) and bool(((_bits(got)[nan] & 0x7fc0) == 0x7fc0).all())       # exponent all ones, quiet bit set
    # same-dtype gathers copy bits, a NaN's included
    got = _gather(corpus.to(DEV), idx, 64, 0.0, F32).cpu()
    assert torch.equal(_bits(got), _bits(_host_batch(corpus, DOC_ROWS, idx, 64, 0.0, F32)))


def test_base_addresses_that_are_not_16_byte_aligned_take_a_narrower_access():
    from multimodaltopicsegmentation_amd import ops
    D, total = 1792, sum(DOC_ROWS)
    corpus = _corpus(D, BF16)
    store = torch.zeros(total * D + 8, dtype=BF16, device=DEV)
    idx = [2, 0, 3, 1]
    ref = _host_batch(corpus, DOC_ROWS, idx, 64, 0.0, BF16)
    for off in (4, 2, 1):                                       # 8-, 4- and 2-byte aligned corpus / batch
        view = store[off:off + total * D].view(total, D)
        view.copy_(corpus)
        out = torch.full((4 * 64 * D + 8,), SENTINEL, dtype=BF16, device=DEV)
        dst = out[off:off + 4 * 64 * D].view(4, 64, D)
        ops.gather_pad(view, _row_start().to(DEV), torch.tensor(idx, dtype=torch.int32, device=DEV), dst, 0.0)
        assert torch.equal(dst.cpu(), ref), off
        assert bool((out[:off] == SENTINEL).all()) and bool((out[off + 4 * 64 * D:] == SENTINEL).all())     # nothing outside dst


def test_offsets_beyond_two_to_the_31():
    """B x Lmax x D = 586 x 2048 x 1792 = 2.15e9 bf16 elements (4.3 GB): an offset kept in 32 bits wraps inside the batch"""
    from multimodaltopicsegmentation_amd import ops
    free = torch.cuda.mem_get_info()[0]
    if free < 6 * 2 ** 30:
        pytest.skip(f'the 4.3 GB batch of the 64-bit offset test needs 6 GB of free device memory; {free / 2 ** 30:.1f} GB are free')
    B, Lmax, D = 586, 2048, 1792
    assert B * Lmax * D > 2 ** 31
    rows = [2048, 700, 3000]
    g = torch.Generator().manual_seed(5)
    corpus = torch.randn(sum(rows), D, generator=g).to(BF16).to(DEV)
    start = _row_start(rows).tolist()
    idx = [(2 * b + 1) % 3 for b in range(B)]
    dst = torch.empty((B, Lmax, D), dtype=BF16, device=DEV)
    dst.fill_(SENTINEL)
    ops.gather_pad(corpus, _row_start(rows).to(DEV), torch.tensor(idx, dtype=torch.int32, device=DEV), dst, 0.0)
    for b in sorted({0, 1, 2, B // 2 - 1, B // 2, B // 2 + 1, B - 3, B - 2, B - 1} | set(range(0, B, 37))):
        d = idx[b]
        n = min(rows[d], Lmax)
        assert torch.equal(dst[b, :n], corpus[start[d]:start[d] + n]), b
        assert n == Lmax or bool((dst[b, n:] == 0).all()), b
    del dst
    torch.cuda.empty_cache()


# ---- ResidentCorpus.batch against the reference collater ----------------------------------------------------------------------

def _to_dev(batch):
    return {k: (v.to(DEV) if isinstance(v, torch.Tensor) and v.is_floating_point() else v) for k, v in batch.items()}


MODES = {'early': dict(), 'late': dict(second=True), 'domain': dict(domain_adapt=True), 'segments': dict(segments=True), 'crf': dict(crf=True)}


@pytest.mark.parametrize('truncate', [True, False])
@pytest.mark.parametrize('wire', ['fp32', 'bf16'])
@pytest.mark.parametrize('mode', list(MODES))
def test_resident_batch_equals_the_collated_batch(mode, wire, truncate):
    from multimodaltopicsegmentation_amd import ResidentCorpus
    ds = _dataset(truncate, **MODES[mode])
    rc = ResidentCorpus(ds, DEV, wire_dtype=wire)
    assert rc.corpus.device.type == 'cuda' and rc.nbytes > 0
    for idx in CASES:
        ref = ds.collater([ds[i] for i in idx])
        got = rc.batch(idx)
        assert set(got) == set(ref)
        for f in ('src_tokens', 'src_tokens2'):
            if ref[f] is None:
                assert got[f] is None
                continue
            want = ref[f].to(torch.bfloat16) if wire == 'bf16' else ref[f]
            assert got[f].device.type == 'cuda' and got[f].dtype == want.dtype and torch.equal(got[f], want.to(DEV)), (f, idx)
        assert got['tgt_tokens'].dtype == torch.float32 and torch.equal(_bits(got['tgt_tokens'].cpu()), _bits(ref['tgt_tokens'])), idx
        assert got['src_lengths'].device.type == 'cpu' and torch.equal(got['src_lengths'], ref['src_lengths'])
        assert torch.equal(got['id'], ref['id']) and got['domain'] == ref['domain']
        assert got.get('src_segments') == ref.get('src_segments')
    if not truncate:
        padded = rc.batch([0, 1], pad_to=20)
        ref = ds.collater([ds[0], ds[1]])
        assert padded['src_tokens'].shape[1] == 20 and padded['tgt_tokens'].shape == (2, 20)
        assert torch.equal(padded['src_tokens'][:, :7].float().cpu(), ref['src_tokens'].to(rc.wire).float()) and bool((padded['src_tokens'][:, 7:] == 0).all())
        assert bool((padded['tgt_tokens'][:, 7:] == -float(ds.minus)).all())


def test_many_batches_in_flight_reuse_the_index_ring_safely():
    """more calls than the pinned index ring has slots, nothing synchronised in between: every batch still holds its own documents"""
    from multimodaltopicsegmentation_amd import ResidentCorpus
    ds = _dataset(False)
    rc = ResidentCorpus(ds, DEV)
    g = torch.Generator().manual_seed(1)
    lists = [torch.randint(0, len(LENGTHS), (int(torch.randint(1, 9, (1,), generator=g)),), generator=g).tolist() for _ in range(50)]
    got = [rc.batch(ix) for ix in lists]
    torch.cuda.synchronize()
    for ix, b in zip(lists, got):
        assert torch.equal(b['src_tokens'].cpu(), ds.collater([ds[i] for i in ix])['src_tokens']), ix


# ---- one training step from a resident batch ----------------------------------------------------------------------------------

TRAIN_LENGTHS = [48, 5, 17, 33, 4, 48, 26, 40, 9, 12, 31, 44, 3, 22, 36, 15]


def _train_dataset(kind, lengths=TRAIN_LENGTHS):
    from multimodaltopicsegmentation_amd import AudioPortionDataset
    d1, d2 = (40, 24) if kind == 'latefusion' else (64, None)
    second = _lines(lengths, D=d2, seed=3) if d2 else None
    return AudioPortionDataset(_lines(lengths, D=d1, seed=2, boundary_p=0.2), {}, CRF=False, truncate=False, second_input=second)


def _build(kind):
    from multimodaltopicsegmentation_amd import BiLSTM, BiLSTMLateFusion, Transformer_segmenter
    if kind == 'transformer':
        return Transformer_segmenter(2, 64, 32, num_layers=2, nheads=4, loss_fn='FocalLoss', window_size=6, compute_dtype='fp32',
                                     max_position_embedding=128, seed=11)
    if kind == 'bilstm':
        return BiLSTM(2, 64, 32, num_layers=2, loss_fn='FocalLoss', compute_dtype='fp32', seed=11)
    return BiLSTMLateFusion(2, [40, 24], 32, num_layers=2, loss_fn='FocalLoss', compute_dtype='fp32', seed=11)


@pytest.mark.parametrize('kind', ['bilstm', 'transformer', 'latefusion'])
def test_a_step_on_a_resident_batch_equals_a_step_on_the_collated_batch(kind):
    from multimodaltopicsegmentation_amd import ResidentCorpus
    from multimodaltopicsegmentation_amd.trainer import NativeTrainer
    ds = _train_dataset(kind)
    rc = ResidentCorpus(ds, DEV)
    m1, m2 = _build(kind).to(DEV), _build(kind).to(DEV)
    t1, t2 = NativeTrainer(m1, lr=1e-3), NativeTrainer(m2, lr=1e-3)
    init = m1.flat.detach().clone()
    for idx in ([0, 1, 2, 3, 4, 6], [5, 7, 7, 9, 10, 12]):
        l1 = t1.step(rc.batch(idx))
        l2 = t2.step(_to_dev(ds.collater([ds[i] for i in idx])))
        assert torch.equal(_bits(l1.detach().float().cpu().view(1)), _bits(l2.detach().float().cpu().view(1)))
    assert torch.equal(m1.flat, m2.flat) and float((m1.flat - init).abs().max()) > 1e-3


# ---- two ranks ----------------------------------------------------------------------------------------------------------------

STEPS, GLOBAL_B = 2, 8


def _dp_lengths(ragged):
    return TRAIN_LENGTHS if ragged else [48] * len(TRAIN_LENGTHS)


def _dp_run(mode, ragged, rank, world):
    """STEPS steps of the transformer on this rank's share of the sampler's global batches; mode 'resident': the rank gathers its own
    documents, 'shard': it collates the global batch and keeps shard_batch's share (what a user had to do before)"""
    from multimodaltopicsegmentation_amd import ResidentCorpus
    from multimodaltopicsegmentation_amd.trainer import NativeTrainer, shard_batch
    ds = _train_dataset('transformer', _dp_lengths(ragged))
    rc = ResidentCorpus(ds, DEV)
    sampler = rc.sampler(GLOBAL_B, rank=rank, world=world, seed=7)
    sampler.set_epoch(1)
    assert len(sampler) == STEPS
    model = _build('transformer').to(DEV)
    tr = NativeTrainer(model, lr=1e-3, optimizer='Adam', token_weighted=ragged)
    losses = []
    for (local, pad_to), g in zip(sampler, sampler.global_batches()):
        if mode == 'resident':
            batch = rc.batch(local, pad_to)
        else:
            batch = _to_dev(shard_batch(ds.collater([ds[i] for i in g.tolist()]), rank, world))
            assert batch['src_tokens'].shape[1] == pad_to and batch['id'].tolist() == local
        losses.append(float(tr.step(batch)))
    torch.cuda.synchronize()
    return model.flat.detach().cpu().clone(), losses, tr


def _dp_worker(rank, world, port, out_dir, ragged):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    torch.cuda.set_device(0)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    out = {}
    for mode in ('resident', 'shard'):
        flat, losses, tr = _dp_run(mode, ragged, rank, world)
        assert tr.world == world and tr._pending == [] and tr.model._grad_hook is not None
        out[mode] = {'flat': flat, 'losses': losses}
    torch.save(out, os.path.join(out_dir, f'r{rank}.pt'))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(600)
@pytest.mark.parametrize('ragged', [True, False])
def test_two_ranks_that_gather_their_own_documents(tmp_path, ragged):
    import torch.multiprocessing as mp
    from tests.test_gpu_dp_step import _free_port
    world = 2
    ctx = mp.spawn(_dp_worker, args=(world, _free_port(), str(tmp_path), ragged), nprocs=world, join=False)
    deadline = time.monotonic() + 240
    try:
        while not ctx.join(timeout=5):                            # raises when a rank exits with a non-zero status
            assert time.monotonic() < deadline, 'the two ranks did not finish in 240 s'
    finally:
        for p in ctx.processes:
            if p.is_alive():
                p.kill()
    assert all(p.exitcode == 0 for p in ctx.processes), [p.exitcode for p in ctx.processes]
    r0, r1 = torch.load(os.path.join(tmp_path, 'r0.pt')), torch.load(os.path.join(tmp_path, 'r1.pt'))
    assert torch.equal(r0['resident']['flat'], r1['resident']['flat'])
    # the same bits as sharding the collated global batch ...
    assert torch.equal(r0['resident']['flat'], r0['shard']['flat']) and torch.equal(r1['resident']['flat'], r1['shard']['flat'])
    assert r0['resident']['losses'] == r0['shard']['losses'] and r1['resident']['losses'] == r1['shard']['losses']
    # ... and the one-process step on the global batch within tests/test_gpu_dp_step.py's bars
    single, losses, _ = _dp_run('resident', ragged, 0, 1)
    init = _build('transformer').flat.detach().clone()
    assert float((single - init).abs().max()) > 1e-3
    diff = (r0['resident']['flat'] - single).abs()
    assert float(diff.max()) <= 2e-5, (float(diff.max()), int(diff.argmax()))
    assert float(diff.mean()) <= 1e-7, float(diff.mean())
