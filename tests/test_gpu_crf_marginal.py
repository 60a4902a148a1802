"""GPU tests of the CRF posterior-marginal decode: mts_crf_marginals (csrc/crf.hip: crf_marg4_kernel for C == 4, crf_marg_kernel for the
other C in 3..8), BiRnnCrf(decode='marginal'), TextSegmenter(crf_decode='marginal') and fit(search_threshold=True) on such a model.

The reference is tests/crf_marginal_oracle.py in fp64 (tests/test_crf_marginal_cpu.py pins it to path enumeration and to the autograd
gradient of oracle.restatement.crf_forward_score).  Every kernel case is launched twice on NaN-filled outputs: the same bits, no NaN left,
exactly 0 past every length.  Bounds, none of them taken from the kernel under test:

  * probabilities sigmoid(score): TOL_DF of tests/test_gpu_crf.py (rtol 1e-3, atol 1e-6);
  * the logit itself against the oracle's logit clamped to +-80: the larger of 2e-3 (rtol 1e-3 on numerator and denominator) and four
    times the error of the same oracle evaluated in fp32 on the CPU on the same inputs (the precedent of
    tests/test_gpu_crf.py::test_crf_nll_at_the_edge_of_the_scaled_recursion; four: the summation order differs);
  * log Z per document: 2e-6 relative (test_gpu_crf.py), with |log Z| floored at 1: the log Z of a short document is a signed sum of
    unit-scale terms that can cancel to any small value while each term carries half an fp32 ulp of its own size, so no fp32 evaluation
    holds 2e-6 of a near-zero sum; test_gpu_crf.py applies its 2e-6 to sums in the thousands and 1e-4 absolute to unit-scale cases;
  * the class sum of the probabilities: 1 within 1e-3 (from that rtol).

Measured worst error / limit on an MI355X: in the docstrings of the tests and in DESIGN.md "CRF posterior-marginal decode".
"""
import numpy as np
import pytest
import torch

from oracle import restatement as R
from tests import crf_marginal_oracle as M
from tests import sweep_oracle as O

pytestmark = pytest.mark.gpu

DEV = 'cuda'
TOL_DF = dict(rtol=1e-3, atol=1e-6)          # tests/test_gpu_crf.py
TOL_LOGZ = 2e-6                              # tests/test_gpu_crf.py (test_crf_long_documents)
LOGIT_FLOOR = 2e-3


@pytest.fixture(scope='module')
def ops():
    from multimodaltopicsegmentation_amd import ops as o
    return o


def _mask_table(trans):
    C = trans.shape[0]
    trans[C - 2, :] = R.IMPOSSIBLE
    trans[:, C - 1] = R.IMPOSSIBLE
    return trans


def _bits(t):
    return t.contiguous().view(torch.int32)


def _run(ops, feats, lengths, trans, cls, want_logz=True):
    """Two launches on NaN-filled outputs, the same bits required -> (scores [B, L], logz [B] or None) on the CPU."""
    B, L, C = feats.shape
    fd, trd = feats.to(DEV), trans.to(DEV)
    li32 = None if lengths is None else torch.as_tensor(lengths, dtype=torch.int32).to(DEV)
    runs = []
    for _ in range(2):
        scores = torch.full((B, L), float('nan'), device=DEV)
        logz = torch.full((B,), float('nan'), device=DEV) if want_logz else None
        ops.crf_marginals(fd, li32, trd, scores, cls=cls, logz=logz)
        runs.append((scores.cpu(), None if logz is None else logz.cpu()))
    assert torch.equal(_bits(runs[0][0]), _bits(runs[1][0])), 'scores, second launch: bits differ'
    if want_logz:
        assert torch.equal(_bits(runs[0][1]), _bits(runs[1][1])), 'logz, second launch: bits differ'
    scores, logz = runs[0]
    assert bool(torch.isfinite(scores).all()), 'a score is not finite (a NaN of the pre-fill, or the recursion left its domain)'
    assert logz is None or bool(torch.isfinite(logz).all())
    for b, n in enumerate([L] * B if lengths is None else lengths):
        assert bool((scores[b, n:] == 0).all()), f'scores of document {b} are not exactly 0 past its length {n}'
    return scores, logz


def _valid(B, L, lengths):
    n = torch.full((B,), L) if lengths is None else torch.as_tensor(lengths)
    return torch.arange(L).unsqueeze(0) < n.unsqueeze(1)


def _judge(scores, logz, ref, ref_z, ref32, valid, label):
    """scores / logz of the kernel against the fp64 oracle (ref, ref_z); ref32 = the oracle's logit in fp32 on the CPU.
    -> (logit err / limit, probability err / limit, log Z err / limit), printed before anything is asserted."""
    want = M.clamped(ref)
    got = scores.double()
    if bool(valid.any()):
        err32 = float((M.clamped(ref32.double()) - want)[valid].abs().max())
        lim = max(LOGIT_FLOOR, 4 * err32)
        err = float((got - want)[valid].abs().max())
        p, pr = torch.sigmoid(got)[valid], torch.sigmoid(ref)[valid]
        perr = (p - pr).abs()
        plim = TOL_DF['atol'] + TOL_DF['rtol'] * pr
        pratio = float((perr / plim).max())
    else:
        err32, lim, err, pratio = 0.0, LOGIT_FLOOR, 0.0, 0.0
    zratio = 0.0
    if logz is not None:
        zratio = float(((logz.double() - ref_z).abs() / (TOL_LOGZ * ref_z.abs().clamp(min=1.0))).max())
    print(f'{label}: logit max err {err:.3e} (oracle in fp32: {err32:.3e}), err / limit {err / lim:.3f}; probability worst err / limit {pratio:.3f}; '
          f'log Z worst err / limit {zratio:.3f}')
    assert err <= lim, f'{label}: logit off by {err:.3e}, limit {lim:.3e}'
    assert pratio <= 1.0, f'{label}: probability err / limit {pratio:.3f}'
    assert zratio <= 1.0, f'{label}: log Z err / limit {zratio:.3f}'
    # beyond the clamp (by more than the bound) the kernel gives the clamp itself
    far = valid & (ref.abs() > M.CLAMP + lim)
    assert torch.equal(got[far], want[far]), f'{label}: a score beyond the clamp is not the clamp'
    return err / lim, pratio, zratio


def _check(ops, feats, lengths, trans, classes, label):
    B, L, _ = feats.shape
    valid = _valid(B, L, lengths)
    out = {}
    for cls in classes:
        ref, ref_z, _ = M.marginals(feats, lengths, trans, cls)
        ref32, _, _ = M.marginals(feats, lengths, trans, cls, dtype=torch.float32)
        scores, logz = _run(ops, feats, lengths, trans, cls)
        _judge(scores, logz, ref, ref_z, ref32, valid, f'{label} cls={cls}')
        out[cls] = (scores, logz)
    return out


def _ragged(B, L, g):
    """Lengths that contain 0, 1 and L, with L at both sides of every block edge the batch reaches."""
    lengths = torch.randint(0, L + 1, (B,), generator=g).tolist()
    lengths[0], lengths[1], lengths[2] = L, 1, 0
    lengths[15] = L                                                    # the last document of the quad kernel's first block
    if B > 16:
        lengths[16] = L                                                # ... and the first of its second
    if B > 64:
        lengths[63], lengths[64] = 1, L                                # the generic kernel's block edge
    return lengths


# ------------------------------------------------------------------------------------------------ 1. C = 4
@pytest.mark.parametrize('L', [1, 9, 33])
@pytest.mark.parametrize('B', [1, 16, 17, 65])
def test_marginals_c4(ops, B, L):
    """crf_marg4_kernel: 16 documents fill a block, 17 crosses it; ragged lengths with 0, 1 and L (B = 1: each of them in turn); both real
    tags; unit-scale inputs.  Measured on an MI355X, the worst of the 12 shapes: logit 1.3e-6 off (0.001 of its limit), probability 0.001
    of its limit, log Z 0.47 of its limit (B = 65, L = 9)."""
    C = 4
    g = torch.Generator().manual_seed(7000 + 100 * B + L)
    length_sets = [[L], [1], [0]] if B == 1 else [_ragged(B, L, g)]
    for lengths in length_sets:
        feats = torch.randn(B, L, C, generator=g)
        trans = _mask_table(torch.randn(C, C, generator=g))
        _check(ops, feats, lengths, trans, (0, 1), f'C=4 B={B} L={L}')


def test_marginals_c4_without_lengths_or_logz(ops):
    """lengths == NULL is every document L long, bit for bit; logz == NULL leaves the scores' bits alone.  Measured on an MI355X: logit
    4.4e-7 off, log Z 0.28 of its limit."""
    B, L, C = 17, 9, 4
    g = torch.Generator().manual_seed(7999)
    feats = torch.randn(B, L, C, generator=g)
    trans = _mask_table(torch.randn(C, C, generator=g))
    for cls in (0, 1):
        (full, full_z), = _check(ops, feats, [L] * B, trans, (cls,), 'C=4 full lengths').values()
        none, none_z = _run(ops, feats, None, trans, cls)
        assert torch.equal(_bits(none), _bits(full)) and torch.equal(_bits(none_z), _bits(full_z))
        bare, _ = _run(ops, feats, None, trans, cls, want_logz=False)
        assert torch.equal(_bits(bare), _bits(full))


# ------------------------------------------------------------------------------------------------ 2. generic C
@pytest.mark.parametrize('B', [1, 65])
@pytest.mark.parametrize('C', [3, 5, 8])
def test_marginals_generic_tagset_sizes(ops, C, B):
    """crf_marg_kernel (one thread per document in the log domain, 64 documents per block), every real tag as cls.  C = 3 has one real
    tag: its logit is +1e4 in the oracle and the clamp, exactly +80, in the kernel.  Measured on an MI355X, the worst of the six cases:
    logit 5.4e-6 off (0.003 of its limit), probability 0.004, log Z 0.20 of their limits."""
    L = 12
    g = torch.Generator().manual_seed(7100 + 10 * C + B)
    lengths = [L] if B == 1 else _ragged(B, L, g)
    feats = torch.randn(B, L, C, generator=g)
    trans = _mask_table(torch.randn(C, C, generator=g))
    out = _check(ops, feats, lengths, trans, tuple(range(C - 2)), f'C={C} B={B}')
    if C == 3:
        assert bool((out[0][0][_valid(B, L, lengths)] == M.CLAMP).all())


def test_marginals_of_start_and_stop_are_the_lower_clamp(ops):
    """cls may be any of 0..C-1: START and STOP carry probability exactly 0, a logit of -1e4 in the oracle and the clamp in the kernels."""
    for C in (4, 5):
        g = torch.Generator().manual_seed(7200 + C)
        feats = torch.randn(3, 7, C, generator=g)
        trans = _mask_table(torch.randn(C, C, generator=g))
        lengths = [7, 3, 0]
        for cls in (C - 2, C - 1):
            ref, _, _ = M.marginals(feats, lengths, trans, cls)
            scores, _ = _run(ops, feats, lengths, trans, cls)
            v = _valid(3, 7, lengths)
            assert bool((ref[v] < -1000).all()) and bool((scores[v] == -M.CLAMP).all())


# ------------------------------------------------------------------------------------------------ 3. the edge of the numeric domain
def _range_case(C):
    """The recipe of tests/test_gpu_crf.py::_range_case at L = 33: emissions uniform in +-30, transitions uniform in +-10."""
    B, L = 8, 33
    g = torch.Generator().manual_seed(5000 + C)
    lengths = [L, L, L, L, 25, 17, 9, L]
    feats = (torch.rand(B, L, C, generator=g) * 2 - 1) * 30
    trans = _mask_table((torch.rand(C, C, generator=g) * 2 - 1) * 10)
    return feats, lengths, trans


@pytest.mark.parametrize('C', [4, 5])
def test_marginals_at_the_edge_of_the_scaled_recursion(ops, C):
    """A step's worst filtered-probability ratio is exp(-80) here, inside the domain include/mts.h states for C == 4 (a normal fp32, above
    exp(-87.3)); C = 5 sends inputs drawn the same way through the log-domain kernel.  Scores finite, within the bounds, and the clamp
    itself where the oracle's logit lies beyond +-80 (_judge).  At these seeds the oracle's largest |logit| is 72.9 (C = 4) and 70.5
    (C = 5), so the clamp is not reached here: C = 3 and the START / STOP test above reach it.  Measured on an MI355X: C = 4 logit 7.9e-6
    off (the oracle in fp32 on the CPU: 1.1e-4; 0.004 of the limit), probability 0.002, log Z 0.07 of their limits; C = 5 logit 1.2e-4 off
    (alpha and beta reach 1e3 in the log domain, one fp32 ulp is 6e-5 there; 0.06 of the limit), probability 0.11, log Z 0.14."""
    feats, lengths, trans = _range_case(C)
    _check(ops, feats, lengths, trans, tuple(range(C - 2)), f'edge C={C}')


# ------------------------------------------------------------------------------------------------ 4. long chain
def test_marginals_long_chain(ops):
    """The corpus's longest and shortest document in one batch: 2 437 dependent steps of the scaled recursion next to 84.  Measured on an
    MI355X: logit 9.5e-7 off (the oracle in fp32 on the CPU: 3.0e-4), probability 0.001, log Z 0.16 of their limits."""
    B, L, C = 2, 2437, 4
    g = torch.Generator().manual_seed(7400)
    feats = torch.randn(B, L, C, generator=g)
    trans = _mask_table(torch.randn(C, C, generator=g))
    _check(ops, feats, [2437, 84], trans, (1,), 'long chain')


# ------------------------------------------------------------------------------------------------ 5. against mts_crf_nll
@pytest.mark.parametrize('C', [4, 5])
def test_marginals_equal_the_nll_gradient(ops, C):
    """d NLL / d feats = (P(y_t = i) - onehot(gold)) / B: with B = 16 undoing the 1 / B is exact, so 16 dfeats[..., cls] + onehot(gold) from
    mts_crf_nll is the probability sigmoid(score_cls) (TOL_DF), and the probabilities of all C tags sum to 1 within 1e-3.  Measured on an
    MI355X: 0.007 (C = 4) and 0.004 (C = 5) of the limit; class sum off 1 by 2.2e-16 and 7.8e-7."""
    B, L = 16, 21
    g = torch.Generator().manual_seed(7500 + C)
    lengths = _ragged(B, L, g)
    feats = torch.randn(B, L, C, generator=g)
    trans = _mask_table(torch.randn(C, C, generator=g))
    tags = torch.zeros(B, L)
    for b, n in enumerate(lengths):
        tags[b, :n] = torch.randint(0, C - 2, (n,), generator=g).float()
    df = torch.full((B, L, C), float('nan'), device=DEV)
    dt = torch.empty(C, C, device=DEV)
    loss = torch.empty(2, device=DEV)
    ops.crf_nll(feats.to(DEV), tags.to(DEV), torch.as_tensor(lengths, dtype=torch.int32).to(DEV), trans.to(DEV), loss, df, dt)
    df = df.cpu().double()
    v = _valid(B, L, lengths)
    total = torch.zeros(B, L, dtype=torch.float64)
    worst = 0.0
    for cls in range(C):
        scores, _ = _run(ops, feats, lengths, trans, cls)
        p = torch.sigmoid(scores.double())
        total += p
        want = 16.0 * df[:, :, cls] + (tags == cls).double()
        lim = TOL_DF['atol'] + TOL_DF['rtol'] * want.abs()
        worst = max(worst, float(((p - want).abs() / lim)[v].max()))
    print(f'C = {C}: probability against 16 dfeats + onehot: worst err / limit {worst:.3f}; class sum off 1 by {float((total - 1)[v].abs().max()):.3e}')
    assert worst <= 1.0
    assert float((total - 1)[v].abs().max()) <= 1e-3


# ------------------------------------------------------------------------------------------------ model and harness
VAL = ((4, 40, [40, 23, 5, 31]), (3, 29, [29, 2, 17]))        # the batches of tests/test_gpu_threshold_sweep.py::_val_batches
MODEL_SEED = 25       # chosen on the CPU (oracle.restatement's encoder): no oracle probability within 7e-3 of 0.3, 0.4 or 0.5, and the lists differ


def _val_batches():
    g = torch.Generator().manual_seed(77)
    out = []
    for B, L, lengths in VAL:
        out.append({'src_tokens': torch.randn(B, L, 64, generator=g).to(DEV), 'src_lengths': torch.tensor(lengths),
                    'tgt_tokens': (torch.rand(B, L, generator=g) < 0.2).float().to(DEV), 'src_tokens2': None, 'domain': None})
    return out


def _crf(dtype='fp32', **kw):
    from multimodaltopicsegmentation_amd import BiRnnCrf
    return BiRnnCrf(2, 64, 32, num_layers=1, compute_dtype=dtype, seed=MODEL_SEED, **kw).to(DEV)


def _model_oracle(m, batch):
    """The oracle on the model's OWN fp32 emissions (what loss_and_grad returns) -> (logit fp64, logit of the fp32 oracle, valid)."""
    lengths = batch['src_lengths'].tolist()
    with torch.no_grad():
        feats = m.loss_and_grad(batch['src_tokens'], batch['src_lengths'], batch['tgt_tokens'], False)[1].float().cpu().clone()
    trans = m.state_dict()['crf.transitions'].detach().float().cpu()
    ref, ref_z, _ = M.marginals(feats, lengths, trans, 1)
    ref32, _, _ = M.marginals(feats, lengths, trans, 1, dtype=torch.float32)
    return ref, ref_z, ref32, _valid(feats.shape[0], feats.shape[1], lengths)


@pytest.mark.parametrize('dtype', ['fp32', 'bf16'])
def test_model_scores(dtype):
    """BiRnnCrf(decode='marginal'): forward's and marginal_scores' [B, Lq, 1] against the oracle on the model's own emissions (the encoder's
    bf16 error is not the new kernel's); the default-decode model gives the same marginal_scores, bit for bit.  Measured on an MI355X:
    logit at most 5.6e-7 off in either dtype."""
    m, plain = _crf(dtype, decode='marginal').eval(), _crf(dtype).eval()
    for bi, batch in enumerate(_val_batches()):
        B, L, lengths = VAL[bi]
        ref, ref_z, ref32, valid = _model_oracle(m, batch)
        scores, tags = m(batch['src_tokens'], batch['src_lengths'])
        assert scores.shape == (B, L, 1) and scores.dtype == torch.float32
        again = m.marginal_scores(batch['src_tokens'], batch['src_lengths'])
        other = plain.marginal_scores(batch['src_tokens'], batch['src_lengths'])
        assert torch.equal(_bits(again), _bits(scores)) and torch.equal(_bits(other), _bits(scores))
        s = scores.cpu().view(B, L)
        assert bool((s[~valid] == 0).all())
        _judge(s, None, ref, ref_z, ref32, valid, f'model {dtype} batch {bi}')
        assert [len(t) for t in tags] == lengths and all(isinstance(v, bool) for t in tags for v in t)


def test_model_decode_lists():
    """forward's bool lists at th = 0.3 and 0.5 (argument) and through .th equal the oracle's prob > th exactly, no position exempted: the
    seed is one at which no oracle probability lies within 1e-3 of a tested threshold (asserted)."""
    m = _crf('fp32', decode='marginal').eval()
    for bi, batch in enumerate(_val_batches()):
        lengths = VAL[bi][2]
        ref, _, _, _ = _model_oracle(m, batch)
        p = torch.sigmoid(ref)
        for th in (0.3, 0.5):
            gap = min(float((p[b, :n] - th).abs().min()) for b, n in enumerate(lengths))
            assert gap > 1e-3, f'an oracle probability lies {gap:.2e} from the threshold {th}: choose another seed'
            want = [(p[b, :n] > th).tolist() for b, n in enumerate(lengths)]
            assert m.th is None
            assert m(batch['src_tokens'], batch['src_lengths'], th)[1] == want
            m.th = th                                                  # .th wins over the argument
            assert m(batch['src_tokens'], batch['src_lengths'], 0.99)[1] == want
            assert m(batch['src_tokens'], batch['src_lengths'])[1] == want
            m.th = None
        default = [(p[b, :n] > 0.4).tolist() for b, n in enumerate(lengths)]
        if min(float((p[b, :n] - 0.4).abs().min()) for b, n in enumerate(lengths)) > 1e-3:
            assert m(batch['src_tokens'], batch['src_lengths'])[1] == default          # the argument's default, as BiLSTM.forward


def test_default_model_is_untouched():
    """A model built without the new argument and one built with decode='viterbi': forward (with and without the ignored threshold), loss
    and the state_dict keys, bit for bit."""
    from multimodaltopicsegmentation_amd import BiRnnCrf
    a = BiRnnCrf(2, 64, 32, num_layers=1, compute_dtype='fp32', seed=MODEL_SEED).to(DEV).eval()
    b = _crf('fp32', decode='viterbi').eval()
    c = _crf('fp32', decode='marginal').eval()
    assert list(a.state_dict().keys()) == list(b.state_dict().keys()) == list(c.state_dict().keys())
    assert all(torch.equal(v, c.state_dict()[k]) for k, v in a.state_dict().items())
    for bi, batch in enumerate(_val_batches()):
        x, n, y = batch['src_tokens'], batch['src_lengths'], batch['tgt_tokens']
        sa, pa = a(x, n)
        sb, pb = b(x, n)
        sb2, pb2 = b(x, n, 0.9)
        assert sa.shape == (VAL[bi][0],) and isinstance(pa[0][0], int)
        assert torch.equal(_bits(sa), _bits(sb)) and torch.equal(_bits(sa), _bits(sb2)) and pa == pb == pb2
        with torch.no_grad():
            la, lb, lc = a.loss(x, n, y), b.loss(x, n, y), c.loss(x, n, y)
        assert torch.equal(_bits(la.view(1)), _bits(lb.view(1))) and torch.equal(_bits(la.view(1)), _bits(lc.view(1)))


def _expected(scores_d, targets, lengths, device_values):
    """Per threshold: decode on the device, then the host metrics per document -> floats [B][T] of (Pk, WD, F1)."""
    from multimodaltopicsegmentation_amd import ops
    B, L, _ = scores_d.shape
    li32 = torch.tensor(lengths, dtype=torch.int32, device=DEV)
    tags = torch.empty(B, L, dtype=torch.uint8, device=DEV)
    fl = [[None] * len(device_values) for _ in range(B)]
    tgt = targets.numpy()
    for j, th in enumerate(device_values):
        ops.greedy_decode(scores_d, li32, float(th), tags)
        tags_h = tags.cpu().numpy()
        for b, n in enumerate(lengths):
            fl[b][j] = O.via_metrics(tags_h[b, :n], tgt[b, :n], False)
    return fl


def _segmenter(**kw):
    from multimodaltopicsegmentation_amd import TextSegmenter
    torch.manual_seed(3)
    return TextSegmenter(2, 64, 32, architecture='biLSTMCRF', crf_decode='marginal', **kw).to(DEV)


@pytest.mark.parametrize('metric', ['Pk', 'WD', 'F1'])
def test_textsegmenter_validation_epoch_hook(metric):
    """The pattern of tests/test_gpu_threshold_sweep.py::test_textsegmenter_validation_epoch_hook on the CRF tagger: the hook's row is the
    host oracle's selection, a twin tested AT a grid value reports that row of the table, all_scores collects [Lq, 1] rows, predict_step
    returns the bool lists."""
    from multimodaltopicsegmentation_amd import DEFAULT_THRESHOLDS, ThresholdSweep
    ts = _segmenter(search_threshold=True, metric=metric)
    batches = _val_batches()
    per_doc = []
    for bi, batch in enumerate(batches):
        assert ts.validation_step(batch, bi) is None
        scores, _ = ts.model(batch['src_tokens'], batch['src_lengths'])
        per_doc.extend(_expected(scores.contiguous(), batch['tgt_tokens'].cpu(), batch['src_lengths'].tolist(), DEFAULT_THRESHOLDS))
    assert len(ts.losses) == 7 and len(ts.targets) == 7 and ts.losses[1].shape == (23, 1)
    want = O.select(O.mean_table(per_doc, DEFAULT_THRESHOLDS), metric)
    got = ts.on_validation_epoch_end()
    assert got == want, (got, want)
    assert ts.best_th == want['threshold'] and want['threshold'] in [float(t) for t in DEFAULT_THRESHOLDS]
    assert ts._sweep.counts().shape[0] == 0

    j = 7
    th = float(DEFAULT_THRESHOLDS[j])
    twin = _segmenter(threshold=th, metric=metric, all_scores=True)
    twin.load_state_dict(ts.state_dict())
    one = ThresholdSweep()
    sc, _ = ts.model(batches[0]['src_tokens'], batches[0]['src_lengths'])
    one.add(sc, batches[0]['tgt_tokens'], batches[0]['src_lengths'])
    row = one.table()
    res = twin.test_step(batches[0], 0)
    key = {'F1': 'F1_loss', 'WD': 'WD_loss'}.get(metric, 'Pk_loss')
    res[key] = res.pop('test_loss')
    assert res['threshold'] == th
    assert (res['Pk_loss'], res['WD_loss'], res['F1_loss']) == (row['Pk_loss'][j], row['WD_loss'][j], row['F1_loss'][j])
    # all_scores: one [Lq, 1] row per document as for the other taggers (Lq = the batch's longest document), exactly 0 past its length
    assert len(twin.scores) == 4
    for b, n in enumerate(VAL[0][2]):
        assert twin.scores[b].shape == (40, 1) and np.array_equal(twin.scores[b], sc[b].cpu().numpy()) and not twin.scores[b][n:].any()
    tags = twin.predict_step(batches[0], 0)
    assert [len(t) for t in tags] == VAL[0][2] and tags == twin.model(batches[0]['src_tokens'], batches[0]['src_lengths'])[1]


TRAIN_LENGTHS = [40, 5, 17, 33, 6, 38, 26, 9]
VAL_LENGTHS = [21, 5, 40, 8, 13, 35]


def _corpus(lengths, seed):
    from multimodaltopicsegmentation_amd import AudioPortionDataset, ResidentCorpus
    from tests.test_resident_corpus_cpu import _lines
    return ResidentCorpus(AudioPortionDataset(_lines(lengths, D=64, seed=seed, boundary_p=0.2), {}, CRF=True, truncate=False), DEV)


@pytest.mark.parametrize('metric', ['Pk', 'scaiano'])
def test_fit_searches_a_threshold_for_the_crf_tagger(metric):
    """fit(search_threshold=True) for 2 epochs: every record carries a grid threshold, model.th is set, the last epoch's row is that of an
    independent sweep over the validation corpus; the same call on a default-decode model is still refused."""
    from multimodaltopicsegmentation_amd import DEFAULT_THRESHOLDS, ThresholdSweep, fit
    from multimodaltopicsegmentation_amd.trainer import NativeTrainer
    train, val = _corpus(TRAIN_LENGTHS, 2), _corpus(VAL_LENGTHS, 6)
    model = _crf('fp32', decode='marginal')
    before = model.flat.detach().clone()
    out = fit(NativeTrainer(model, lr=1e-3), train, val, batch_size=4, max_epochs=2, seed=5, search_threshold=True, metric=metric,
              restore_best=False)
    grid = [float(t) for t in DEFAULT_THRESHOLDS]
    assert len(out['epochs']) == 2 and all(r['threshold'] in grid for r in out['epochs']) and out['threshold'] in grid
    assert model.th == out['epochs'][-1]['threshold'] and not torch.equal(model.flat, before)
    model.eval()
    sweep = ThresholdSweep(metric=metric)
    for s in range(0, len(val), 4):
        batch = val.batch(list(range(s, min(s + 4, len(val)))))
        sweep.add(model(batch['src_tokens'], batch['src_lengths'])[0], batch['tgt_tokens'], batch['src_lengths'])
    row = sweep.best(metric)
    assert {k: out['epochs'][-1][k] for k in row} == row
    plain = _crf('fp32')
    with pytest.raises(NotImplementedError, match='biLSTMCRF'):
        fit(NativeTrainer(plain, lr=1e-3), train, val, batch_size=4, max_epochs=1, search_threshold=True, metric=metric)
