"""CPU tests of the cosine auxiliary segment loss: the fp64 oracle (tests/cosine_oracle.py) against the reference's fixture g21, the host
table (ops.segment_table) against a literal Python-slicing restatement, its ValueError / IndexError cases, the reference's error messages,
the collater's opt-in 'src_segments' on both collater paths, shard_batch and the NativeTrainer keyword."""
import numpy as np
import pytest
import torch

from tests import cosine_oracle as O
from tests.helpers import load, seeded_param

CASES = ('fo', 'bc', 'ce', 'lf')


def case(g, c, dtype=torch.float64):
    """-> dict with the fixture's inputs as tensors, the segment lists and the regenerated weights (helpers.seeded_param)"""
    D1, D2, H, NL = (int(v) for v in g[f'{c}_cfg'])
    late = str(g[f'{c}_cls']) == 'BiLSTMLateFusion'
    loss_fn = str(g[f'{c}_loss_fn'])
    n_out = 2 if loss_fn == 'CrossEntropy' else 1
    shapes = O.param_shapes((D1, D2) if late else D1, H, NL, n_out, late)
    seed = int(g[f'{c}_seed'])
    off, flat = g[f'{c}_seg_off'], g[f'{c}_seg_flat']
    segments = [flat[off[b]:off[b + 1]].tolist() for b in range(len(off) - 1)]
    xs = [torch.from_numpy(g[f'{c}_x{i}']).to(dtype) for i in ((1, 2) if late else (1,))]
    return dict(D=(D1, D2) if late else D1, H=H, NL=NL, late=late, loss_fn=loss_fn, n_out=n_out, segments=segments, xs=xs, seed=seed,
                lengths=torch.from_numpy(g[f'{c}_lengths']), tags=torch.from_numpy(g[f'{c}_tags']),
                p={n: torch.from_numpy(seeded_param(n, s, seed)).to(dtype) for n, s in shapes.items()})


def test_fixture_covers_the_cases_it_must():
    g = load('g21_cosine_loss')
    spans, has_empty_doc, last_eq, last_lt, len1, any_neg = [], False, False, False, False, False
    for c in CASES:
        cs = case(g, c)
        for n, ends in zip(cs['lengths'].tolist(), cs['segments']):
            has_empty_doc |= not ends
            len1 |= n == 1
            if ends:
                last_eq |= ends[-1] == n
                last_lt |= ends[-1] < n
                spans += list(np.diff([0] + ends))
        cos, ne, npos = g[f'{c}_cos'], g[f'{c}_cos_nonempty'], int(g[f'{c}_npos'])
        assert not ne[:npos].any() and np.abs(cos[ne]).min() >= 0.05                    # the generator's condition
        assert (cos[npos:][~ne[npos:]] == 0).all()                                       # empty partner: cos exactly 0
        any_neg |= bool((cos[ne] < 0).any())
        assert (cs['tags'].numpy()[np.arange(cs['tags'].shape[1])[None] >= cs['lengths'].numpy()[:, None]] == (0 if c == 'bc' else -1)).all()
    assert 1 in spans and any(s % 2 == 1 and s > 1 for s in spans) and has_empty_doc and last_eq and last_lt and len1 and any_neg
    assert int(g['bc_cfg'][2]) == 12                                                     # H = 12: stored padded by the product


@pytest.mark.parametrize('c', CASES)
def test_oracle_matches_reference_fixture(c):
    g = load('g21_cosine_loss')
    cs = case(g, c)
    for t in cs['p'].values():
        t.requires_grad_(True)
    xs = [x.clone().requires_grad_(True) for x in cs['xs']]
    loss, cos, _ = O.loss(tuple(xs) if cs['late'] else xs[0], cs['lengths'], cs['tags'].double(), cs['segments'], cs['p'], cs['loss_fn'])
    want = float(g[f'{c}_loss'])
    assert abs(loss.item() - want) < 1e-6 * max(1.0, abs(want))
    assert cos.shape == g[f'{c}_cos'].shape and np.abs(cos.detach().numpy() - g[f'{c}_cos']).max() < 1e-6
    loss.backward()
    for i, x in enumerate(xs):
        gx = g[f'{c}_gx{i + 1}']
        assert np.abs(x.grad.numpy() - gx).max() <= 1e-5 * np.abs(gx).max()
    for n, t in cs['p'].items():
        w = g[f'{c}_g.{n}']
        assert np.abs(t.grad.numpy() - w).max() <= 1e-5 * np.abs(w).max(), n               # fp64 against the reference's fp32
    # no pair: the cosine term is the int 0 and the main loss is still unmasked
    xs0 = [x.clone().requires_grad_(True) for x in cs['xs']]
    p0 = {n: t.detach() for n, t in cs['p'].items()}
    loss0, cos0, scores = O.loss(tuple(xs0) if cs['late'] else xs0[0], cs['lengths'], cs['tags'].double(), [[] for _ in cs['segments']], p0, cs['loss_fn'])
    assert cos0.numel() == 0 and abs(loss0.item() - float(g[f'{c}_p0_loss'])) < 1e-6 * max(1.0, abs(float(g[f'{c}_p0_loss'])))
    assert abs(loss0.item() - O.main_loss(scores, cs['tags'].double(), cs['loss_fn']).item()) == 0.0
    loss0.backward()
    assert np.abs(xs0[0].grad.numpy() - g[f'{c}_p0_gx1']).max() <= 1e-5 * np.abs(g[f'{c}_p0_gx1']).max()


def _slicing_pairs(L, lengths, segments):
    """The reference's aggregate_embeddings on row NUMBERS instead of embeddings: -> [(rows of a, rows of b, target)], positives first."""
    out = []
    for positive in (True, False):
        for b, ends in enumerate(segments):
            rows = list(range(b * L, b * L + lengths[b]))
            prev = 0
            for j, s in enumerate(ends):
                seg = rows[prev:s]
                if positive:
                    if len(seg) > 1:
                        out.append((seg[::2], seg[1::2], 1))
                else:
                    try:
                        nxt = rows[s:ends[j + 1]]
                    except IndexError:
                        nxt = rows[s:]
                    out.append((seg, nxt, -1))
                prev = s
    return out


def _table_pairs(tab):
    seg, out = tab.seg, []

    def rows(s, parity=None):
        r = list(range(seg[s, 0] * tab.L + seg[s, 1], seg[s, 0] * tab.L + seg[s, 2]))
        return r if parity is None else r[parity::2]
    for a, b, t, _ in tab.pair.tolist():
        out.append((rows(a, 0), rows(a, 1), 1) if t > 0 else (rows(a), rows(b), -1))
    return out


def _random_segments(rng, lengths):
    out = []
    for n in lengths:
        k = int(rng.integers(0, min(n, 6) + 1))
        out.append(sorted(rng.choice(np.arange(1, n + 1), size=k, replace=False).tolist()) if k else [])
    return out


def test_segment_table_matches_python_slicing():
    from multimodaltopicsegmentation_amd import ops
    rng = np.random.default_rng(5)
    for trial in range(40):
        B = int(rng.integers(1, 7))
        lengths = [int(v) for v in rng.integers(1, 20, size=B)]
        L = max(lengths) + (trial % 2)                                   # the padded length may exceed every document
        segments = _random_segments(rng, lengths)
        tab = ops.segment_table(segments + [[99]] * (trial % 3), torch.tensor(lengths), B, L)       # entries past B are ignored
        assert tab.seg.dtype == tab.pair.dtype == tab.row_map.dtype == np.int32
        assert _table_pairs(tab) == _slicing_pairs(L, lengths, segments)
        assert tab.n_pair == sum(len(e) for e in segments) + sum(1 for n, e in zip(lengths, segments) for w in np.diff([0] + e) if w > 1)
        # row map: every row of a document with a list is in exactly the segment that contains it, with its parity; every other row is -1
        want = np.full(B * L, -1)
        for s, (doc, begin, end, tail, pos, nf, ns, _) in enumerate(tab.seg.tolist()):
            want[doc * L + begin:doc * L + end] = 2 * s + (np.arange(end - begin) & 1)
            assert tail == (nf == -1) and (pos >= 0) == (not tail and end - begin > 1)
            if nf >= 0:
                assert tab.pair[nf].tolist()[:3] == [s, s + 1, -1] and tab.seg[s + 1, 6] == nf and tab.seg[s + 1, 0] == doc
            if pos >= 0:
                assert tab.pair[pos].tolist()[:3] == [s, s, 1]
        assert (tab.row_map == want).all()
        for b, (n, e) in enumerate(zip(lengths, segments)):
            m = tab.row_map[b * L:(b + 1) * L]
            assert (m[n:] == -1).all() and ((m[:n] >= 0).all() if e else (m == -1).all())
    empty = ops.segment_table([[], []], torch.tensor([3, 2]), 2, 3)
    assert empty.n_seg == 0 and empty.n_pair == 0 and empty.seg.shape == (0, 8) and empty.pair.shape == (0, 4) and (empty.row_map == -1).all()
    one = ops.segment_table([[1]], torch.tensor([1]), 1, 1)               # a length-1 document: one pair with an empty partner
    assert one.n_pair == 1 and one.seg.tolist() == [[0, 0, 1, 0, -1, 0, -1, 0], [0, 1, 1, 1, -1, -1, 0, 0]]


def test_segment_table_validation():
    from multimodaltopicsegmentation_amd import ops
    g = load('g21_cosine_loss')
    lengths = torch.tensor([5, 3])
    with pytest.raises(IndexError) as e:                                  # shorter than the batch: as upstream
        ops.segment_table([[2]], lengths, 2, 5)
    assert type(e.value).__name__ == str(g['err_short_type']) and str(e.value) == str(g['err_short_msg'])
    for bad in ([[0, 2], []], [[2, 2], []], [[3, 2], []], [[6], []], [[2], [4]], [[-1], []], [[2.5], []], [[True], []]):
        with pytest.raises(ValueError):                                   # the documented divergence: upstream slices silently
            ops.segment_table(bad, lengths, 2, 5)
    with pytest.raises(ValueError):
        ops.segment_table([[2], [1]], torch.tensor([5, 3, 1]), 2, 5)
    with pytest.raises(ValueError):
        ops.segment_table(7, lengths, 2, 5)
    assert ops.segment_table([[5], [3]], lengths, 2, 5).n_pair == 4       # s == length is valid: two positive + two negative pairs
    assert ops.segment_table([[4], [2]], torch.tensor([9, 3]), 2, 4).n_pair == 4      # a length past the padded length is clamped to it
    with pytest.raises(ValueError):
        ops.segment_table([[5], []], torch.tensor([9, 3]), 2, 4)


def test_reference_error_messages_are_reproduced():
    from multimodaltopicsegmentation_amd import BiLSTM
    g = load('g21_cosine_loss')
    cs = case(g, 'bc', torch.float32)
    x, lengths, tags = cs['xs'][0], cs['lengths'], cs['tags']
    long_tags = torch.cat((tags, torch.full((tags.shape[0], 1), -1.0)), dim=1)
    for loss_fn in ('FocalLoss', 'BinaryCrossEntropy', 'CrossEntropy'):
        m = BiLSTM(2, cs['D'], cs['H'], cs['NL'], loss_fn=loss_fn, seed=1)
        assert str(g[f'err_tags_{loss_fn}_type']) == 'ValueError'
        with pytest.raises(ValueError) as e:
            m._segment_tables(cs['segments'], x, lengths, long_tags)
        assert str(e.value) == str(g[f'err_tags_{loss_fn}_msg'])
        with pytest.raises(IndexError):
            m._segment_tables(cs['segments'][:-1], x, lengths, tags)
        pad = tags.clone()
        for b, n in enumerate(lengths.tolist()):
            pad[b, n:] = -1
        if loss_fn == 'BinaryCrossEntropy':                                # nn.BCELoss over every position refuses the pad -1
            with pytest.raises(RuntimeError) as e:
                m._segment_tables(cs['segments'], x, lengths, pad)
            assert type(e.value).__name__ == str(g['err_bce_pad_type']) and str(e.value) == str(g['err_bce_pad_msg'])
        else:
            assert m._segment_tables(cs['segments'], x, lengths, pad).n_pair == len(g['bc_cos'])
        assert m._segment_tables(cs['segments'], x, lengths, tags).n_pair == len(g['bc_cos'])


def _lines(rng, lengths, D=8, D2=None):
    lines, second = [], []
    for i, n in enumerate(lengths):
        t = (rng.random(n) < 0.3).astype(np.float32)
        t[-1] = 0.0
        if i == 1:
            t[:] = 0.0                                                     # a document without a boundary -> []
        lines.append((torch.from_numpy(rng.standard_normal((n, D)).astype(np.float32)), t.tolist(), f'doc{i}'))
        if D2:
            second.append((torch.from_numpy(rng.standard_normal((n, D2)).astype(np.float32)), t.tolist(), f'doc{i}'))
    return lines, second or None


@pytest.mark.parametrize('truncate', [False, True])
def test_collater_adds_src_segments_on_both_paths(truncate):
    from multimodaltopicsegmentation_amd import ops
    from multimodaltopicsegmentation_amd.encoder_dataset import AudioPortionDataset
    rng = np.random.default_rng(11)
    lengths = [9, 6, 1, 14]
    lines, second = _lines(rng, lengths, D2=4)
    kw = dict(CRF=False, truncate=truncate, truncate_value=7, second_input=second)
    plain = AudioPortionDataset(lines, None, **kw)
    keys = set(plain.collater([plain[i] for i in range(4)]))
    assert keys == {'id', 'src_tokens', 'src_lengths', 'tgt_tokens', 'src_tokens2', 'domain'}          # off by default: the reference's keys
    for ring in (False, True):
        off = AudioPortionDataset(lines, None, pin_memory=ring, **kw)
        assert set(off.collater(off.__getitems__([0, 1, 2, 3]))) == keys
        ds = AudioPortionDataset(lines, None, pin_memory=ring, segments=True, **kw)
        batches = [ds.collater([ds[i] for i in range(4)]), ds.collater(ds.__getitems__([0, 1, 2, 3]))]   # per-sample path, batched fetch
        for batch in batches:
            assert set(batch) == keys | {'src_segments'}
            segs, lens = batch['src_segments'], batch['src_lengths'].tolist()
            assert lens == [min(n, 7) for n in lengths] if truncate else lens == lengths
            for b, n in enumerate(lens):
                assert segs[b] == [t + 1 for t in range(n) if lines[b][1][t] == 1]
            assert segs[1] == [] and segs[2] == []
            tab = ops.segment_table(segs, batch['src_lengths'], 4, batch['src_tokens'].shape[1])     # what the collater makes is always valid
            assert tab.n_pair >= sum(len(s) for s in segs)
        assert batches[0]['src_segments'] == batches[1]['src_segments']


def test_shard_batch_and_prefetcher_carry_the_segments():
    from multimodaltopicsegmentation_amd.prefetch import DevicePrefetcher
    from multimodaltopicsegmentation_amd.trainer import shard_batch
    segs = [[1, 3], [], [2], [4, 5], [1]]
    batch = {'src_tokens': torch.zeros(5, 6, 8), 'src_lengths': torch.tensor([6, 2, 3, 5, 1]), 'tgt_tokens': torch.zeros(5, 6),
             'src_tokens2': None, 'domain': None, 'src_segments': segs}
    assert shard_batch(batch, 0, 1) is batch
    for world in (2, 3):
        got = [shard_batch(batch, r, world) for r in range(world)]
        for r, sh in enumerate(got):
            assert sh['src_segments'] == segs[r::world] and sh['src_lengths'].tolist() == batch['src_lengths'][r::world].tolist()
            assert len(sh['src_segments']) == sh['src_tokens'].shape[0]
    out = list(DevicePrefetcher([batch], 'cpu'))
    assert out[0]['src_segments'] is segs


def test_trainer_keyword():
    from multimodaltopicsegmentation_amd import BiLSTM
    from multimodaltopicsegmentation_amd.trainer import NativeTrainer
    m = BiLSTM(2, 16, 8, 1, loss_fn='FocalLoss', seed=1)
    assert NativeTrainer(m).cosine_loss is False and NativeTrainer(m, cosine_loss=True).cosine_loss is True
    with pytest.raises(ValueError, match='token_weighted'):
        NativeTrainer(m, cosine_loss=True, token_weighted=True)
    # models whose loss_and_grad takes no segments keep their refusal: named at construction, not a TypeError inside a step
    from multimodaltopicsegmentation_amd import BiLSTMLateFusion, BiRnnCrf, SheikhBiLSTM, SwitchBiLSTM
    assert NativeTrainer(BiLSTMLateFusion(2, [16, 8], 8, 1, loss_fn='FocalLoss', seed=1), cosine_loss=True).cosine_loss
    for other in (SwitchBiLSTM(2, 16, 8, 1, loss_fn='FocalLoss', seed=1), BiRnnCrf(2, 16, 8, 1, seed=1), SheikhBiLSTM(2, 16, 8, 1, seed=1)):
        assert NativeTrainer(other).cosine_loss is False
        with pytest.raises(NotImplementedError, match='segments'):
            NativeTrainer(other, cosine_loss=True)


def test_device_tables_validate_on_every_call():
    """ops.segment_tables keeps nothing between calls: a list that only LOOKS like one seen before ([True] ~ [1], [2.0] ~ [2]) is refused"""
    from multimodaltopicsegmentation_amd import ops
    lengths = torch.tensor([5, 3])
    ok = ops.segment_tables([[1, 2], [2]], lengths, 2, 5, 'cpu')
    assert ok.n_pair == 4 and ok.seg.numel() == ok.n_seg * 8 and ok.pair.numel() == 16 and ok.row_map.numel() == 10
    for bad in ([[True, 2], [2]], [[1.0, 2.0], [2]], [[1, 2], [2.0]]):
        with pytest.raises(ValueError):
            ops.segment_tables(bad, lengths, 2, 5, 'cpu')
