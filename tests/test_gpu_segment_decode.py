"""mts_segment_decode (csrc/segment_decode.hip) against the host restatement of tests/segment_decode_oracle.py.  Every comparison is ``==``:
the test reads the kernel's ``prob`` back, forms the fixed-point weights on the host, runs the oracle and holds tags, segment table and
counts to it, every padded element included -- the decode is integers after decode_prob, so there are no tolerances.  The outputs are
filled with a pattern before every call, so an element the kernel did not write shows.

Shapes: the lengths at which the kernel takes another path -- around the 64-sentence mask words, the 256-thread trips, the runs of
min(m, 64) positions, n = 2m - 1 / 2m / 2m + 1 where the eligible interior appears, a document of 65 536 sentences (every mask word, 32
tiles of staged probabilities, the longest ring) -- and an Smax below the count."""
import numpy as np
import pytest
import torch

from tests import segment_decode_oracle as O

pytestmark = pytest.mark.gpu
DEV = 'cuda'
L = 520
LENGTHS = [0, 1, 2, 63, 64, 65, 128, 129, 255, 256, 257, 513]
FIVE = torch.tensor([-2.0, -0.5, 0.0, 0.5, 2.0])


def _ops():
    from multimodaltopicsegmentation_amd import ops
    return ops


def _run(scores, lengths, threshold, m, close_last=True, Smax=None, fill=0xAB, want_tags=True, want_prob=True):
    """-> numpy (tags, prob, seg_end, n_seg); the outputs hold ``fill`` bytes before the launch"""
    ops = _ops()
    B, Lq, _ = scores.shape
    Smax = Lq if Smax is None else Smax
    li = None if lengths is None else torch.tensor(lengths, dtype=torch.int32, device=DEV)
    tags = torch.full((B, Lq), fill, dtype=torch.uint8, device=DEV) if want_tags else None
    prob = torch.full((B, Lq), float('nan'), dtype=torch.float32, device=DEV) if want_prob else None
    seg_end = torch.full((B, Smax), -(fill << 8), dtype=torch.int32, device=DEV)
    n_seg = torch.full((B,), -(fill << 8), dtype=torch.int32, device=DEV)
    ops.segment_decode(scores, li, threshold, seg_end, n_seg, min_segment=m, close_last=close_last, tags=tags, prob=prob)
    torch.cuda.synchronize()
    return (None if tags is None else tags.cpu().numpy(), None if prob is None else prob.cpu().numpy(), seg_end.cpu().numpy(), n_seg.cpu().numpy())


def _scores(B, Lq, n_out, kind, seed):
    g = torch.Generator().manual_seed(seed)
    if kind == 'five':
        s = FIVE[torch.randint(0, 5, (B, Lq, n_out), generator=g)]
    else:
        s = torch.randn(B, Lq, n_out, generator=g) * 1.5
    return s.contiguous().to(DEV)


def _check(got, lengths, threshold, m, close_last, Smax, Lq):
    tags, prob, seg_end, n_seg = got
    B = prob.shape[0]
    ns = [Lq if lengths is None else min(max(int(v), 0), Lq) for v in (lengths if lengths is not None else [Lq] * B)]
    for b, n in enumerate(ns):
        assert (prob[b, n:] == 0).all() and np.isfinite(prob[b]).all() and (prob[b] >= 0).all() and (prob[b] <= 1).all()
    want_tags, want_end, want_n = O.decode(prob, lengths, threshold, m, close_last, Smax)
    assert np.array_equal(n_seg, want_n), (n_seg.tolist(), want_n.tolist())
    assert np.array_equal(tags, want_tags), [b for b in range(B) if not np.array_equal(tags[b], want_tags[b])]
    assert np.array_equal(seg_end, want_end), [b for b in range(B) if not np.array_equal(seg_end[b], want_end[b])]
    return ns, want_tags


@pytest.mark.parametrize('n_out', [1, 2, 3])
@pytest.mark.parametrize('m', [1, 2, 3, 63, 64, 65, 256])
def test_tags_table_and_counts_equal_the_oracle(m, n_out):
    lengths = LENGTHS + [2 * m - 1, 2 * m, 2 * m + 1]
    B = len(lengths)
    boundaries = 0
    for kind, th in (('five', 0.5), ('normal', 0.35)):
        scores = _scores(B, L, n_out, kind, seed=100 * m + n_out)
        for lens in (lengths, None):
            for close_last in (True, False):
                got = _run(scores, lens, th, m, close_last=close_last)
                ns, want_tags = _check(got, lens, th, m, close_last, L, L)
                for b, n in enumerate(ns):
                    assert O.admissible(want_tags[b, :n], m)
                boundaries += int(want_tags.sum())
        # an Smax below the counts: the table is cut, the counts are not
        got = _run(scores, lengths, th, m, Smax=3)
        _check(got, lengths, th, m, True, 3, L)
        assert (got[3] > 3).any() or m > 64
        # tags and prob are optional: the table does not change without them
        bare = _run(scores, lengths, th, m, Smax=3, want_tags=False, want_prob=False)
        assert np.array_equal(bare[2], got[2]) and np.array_equal(bare[3], got[3])
    assert boundaries > 0


def test_ties_between_boundary_sets_are_present_in_the_five_value_scores():
    """the five-value scores hold p == threshold exactly (score 0 -> 0.5): q = 0 there, and the strict compares decide"""
    scores = _scores(4, L, 1, 'five', seed=9)
    tags, prob, _, _ = _run(scores, None, 0.5, 3)
    q = O.fixed_point(prob.reshape(-1), 0.5)
    assert (q == 0).sum() > 100 and (q > 0).any() and (q < 0).any()


@pytest.mark.parametrize('n_out', [1, 2, 3])
def test_at_min_segment_1_the_tags_are_greedy_decode_s_bits(n_out):
    ops = _ops()
    B = len(LENGTHS)
    scores = _scores(B, L, n_out, 'normal', seed=40 + n_out)
    li = torch.tensor(LENGTHS, dtype=torch.int32, device=DEV)
    _, prob, _, _ = _run(scores, LENGTHS, 0.5, 1)
    b, i = 11, 200                                                                       # an entry of the device's own prob, inside its document
    exact = np.float32(prob[b, i])
    below = np.nextafter(exact, np.float32(0))
    assert 0 < below < exact < 1
    for th in (1e-6, 0.5, float(exact), float(below)):
        tags, prob2, _, _ = _run(scores, LENGTHS, th, 1)
        greedy = torch.full((B, L), 7, dtype=torch.uint8, device=DEV)
        ops.greedy_decode(scores, li, th, greedy)
        assert np.array_equal(tags, greedy.cpu().numpy()), th
        assert np.array_equal(prob2.view(np.uint32), prob.view(np.uint32))
        assert np.array_equal(tags, (prob > np.float32(th)) & (np.arange(L)[None, :] < np.array(LENGTHS)[:, None]))
    # equal gives 0 (strict), the predecessor float gives 1: prob holds decode_prob's bits
    assert _run(scores, LENGTHS, float(exact), 1)[0][b, i] == 0 and _run(scores, LENGTHS, float(below), 1)[0][b, i] == 1
    # without lengths every row is L long
    tags, _, _, _ = _run(scores, None, 0.5, 1)
    greedy = torch.empty((B, L), dtype=torch.uint8, device=DEV)
    ops.greedy_decode(scores, None, 0.5, greedy)
    assert np.array_equal(tags, greedy.cpu().numpy())


def test_a_document_of_65536_sentences():
    n = 65536
    high = torch.full((1, n, 1), 4.0, device=DEV)
    tags, prob, seg_end, n_seg = _run(high, None, 0.5, 1)
    assert n_seg.tolist() == [n] and np.array_equal(seg_end[0], np.arange(1, n + 1, dtype=np.int32)) and tags.all()
    # the same document under a minimum length of 1024 sentences, and a random one, against the oracle
    got = _run(high, None, 0.5, 1024)
    _check(got, None, 0.5, 1024, True, n, n)
    assert got[3].tolist() == [n // 1024 - 1 + 1]                                        # boundaries at 1023, 2047, .., 64511 and the last sentence
    rnd = _scores(1, n, 2, 'normal', seed=3)
    for m in (2, 1024):
        got = _run(rnd, [n - 5], 0.4, m, Smax=4096)
        _check(got, [n - 5], 0.4, m, True, 4096, n)


def test_limits_are_refused_before_a_launch():
    ops = _ops()
    one = torch.empty((1, 1), dtype=torch.int32, device=DEV)
    cnt = torch.empty(1, dtype=torch.int32, device=DEV)
    with pytest.raises(NotImplementedError):
        ops.segment_decode(torch.zeros((1, 65537, 1), device=DEV), None, 0.5, one, cnt)
    with pytest.raises(NotImplementedError):
        ops.segment_decode(torch.zeros((1, 8, 1), device=DEV), None, 0.5, one, cnt, min_segment=1025)
    with pytest.raises(NotImplementedError):
        ops.segment_decode(torch.zeros((1, 8, 1), device=DEV), None, 0.5, one, cnt, min_segment=0)
    with pytest.raises(ValueError):
        ops.segment_decode(torch.zeros((1, 8, 5), device=DEV), None, 0.5, one, cnt)
    with pytest.raises(ValueError):
        ops.segment_decode(torch.zeros((1, 8, 1), device=DEV), None, float('nan'), one, cnt, min_segment=2)
    torch.cuda.synchronize()


@pytest.mark.parametrize('m', [1, 3, 65])
def test_two_calls_give_identical_bytes(m):
    scores = _scores(len(LENGTHS), L, 2, 'five', seed=77)
    a = _run(scores, LENGTHS, 0.5, m, fill=0xAB)
    b = _run(scores, LENGTHS, 0.5, m, fill=0x5C)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()
