"""CPU-only: the fp64 oracle of the CRF posterior-marginal decode (tests/crf_marginal_oracle.py) pinned to three independent statements of
the same quantity, and what of mts_crf_marginals / BiRnnCrf(decode=) / TextSegmenter(crf_decode=) can be checked without a GPU: the
symbol, its argument validation (before any device work, as tests/test_abi.py), the constructor errors and the sweep refusal."""
import ctypes

import pytest
import torch

from oracle import restatement as R
from tests import crf_marginal_oracle as M


def _mask_table(trans):
    C = trans.shape[0]
    trans[C - 2, :] = R.IMPOSSIBLE
    trans[:, C - 1] = R.IMPOSSIBLE
    return trans


def _case(C, B, L, seed, lengths=None):
    g = torch.Generator().manual_seed(seed)
    feats = torch.randn(B, L, C, generator=g, dtype=torch.float64)
    trans = _mask_table(torch.randn(C, C, generator=g, dtype=torch.float64))
    return feats, trans, lengths


# ------------------------------------------------------------------------------------------------ the oracle
@pytest.mark.parametrize('C', [3, 4, 5])
def test_oracle_equals_enumeration_over_every_path(C):
    """All C^n paths for n <= 5 with ragged lengths (0 included): logit of every tag and log Z to 1e-12."""
    lengths = [5, 0, 1, 3, 4, 2]
    feats, trans, _ = _case(C, len(lengths), 5, 100 + C)
    for cls in range(C - 2):
        logit, logz, _ = M.marginals(feats, lengths, trans, cls)
        for b, n in enumerate(lengths):
            want, want_z = M.brute_force(feats[b, :n], trans, cls)
            assert abs(float(logz[b] - want_z)) < 1e-12, (C, cls, b)
            # (a lone real tag, C = 3, has logits of 1e4, the IMPOSSIBLE convention: 1e-12 of the value there)
            err = (logit[b, :n] - want).abs() / want.abs().clamp(min=1.0)
            assert n == 0 or float(err.max()) < 1e-12, (C, cls, b, float(err.max()))
            assert bool((logit[b, n:] == 0).all())


@pytest.mark.parametrize('C', [3, 4, 5, 8])
def test_oracle_is_the_gradient_of_the_restated_forward_score(C):
    """sigmoid(logit_cls) = P(y_t = cls | x) = d log Z / d f_t(cls): column cls of the autograd gradient of
    oracle.restatement.crf_forward_score (the code fixture g5 pins to the reference), and log Z is its value."""
    lengths = [12, 0, 1, 7, 12, 3]
    feats, trans, _ = _case(C, len(lengths), 12, 200 + C)
    f = feats.clone().requires_grad_(True)
    mask = R.create_mask(12, torch.as_tensor(lengths)).double()
    z = R.crf_forward_score(f, mask, trans)
    z.sum().backward()
    for cls in range(C):
        logit, logz, lm = M.marginals(feats, lengths, trans, cls)
        assert float((logz - z.detach()).abs().max()) < 1e-12
        p = torch.sigmoid(logit)
        for b, n in enumerate(lengths):
            assert n == 0 or float((p[b, :n] - f.grad[b, :n, cls]).abs().max()) < 1e-12, (C, cls, b)


def test_oracle_with_a_flat_transition_table_is_the_emission_difference():
    """Every transition among real tags, out of START and into STOP equal to 0: the chain factorises and the logit of tag 1 is
    f_t(1) - f_t(0) for two real tags, f_t(1) - lse(f_t(0), f_t(2)) for three."""
    for C in (4, 5):
        g = torch.Generator().manual_seed(300 + C)
        feats = torch.randn(3, 9, C, generator=g, dtype=torch.float64)
        trans = _mask_table(torch.zeros(C, C, dtype=torch.float64))
        lengths = [9, 4, 1]
        logit, _, _ = M.marginals(feats, lengths, trans, 1)
        rest = [i for i in range(C - 2) if i != 1]
        want = feats[:, :, 1] - torch.logsumexp(feats[:, :, rest], dim=-1)
        for b, n in enumerate(lengths):
            assert float((logit[b, :n] - want[b, :n]).abs().max()) < 1e-13, (C, b)


@pytest.mark.parametrize('C', [3, 4, 5, 8])
def test_oracle_marginals_sum_to_one_over_the_real_tags(C):
    lengths = [12, 5, 1]
    feats, trans, _ = _case(C, 3, 12, 400 + C)
    _, _, lm = M.marginals(feats, lengths, trans, 0)
    p = lm.exp()
    for b, n in enumerate(lengths):
        assert float((p[b, :n, :C - 2].sum(-1) - 1).abs().max()) < 1e-12
        assert bool((p[b, :n, C - 2:] == 0).all())                    # START and STOP carry exactly 0


def test_oracle_in_fp32_is_the_same_function():
    feats, trans, _ = _case(4, 2, 9, 500)
    a, za, _ = M.marginals(feats, [9, 4], trans, 1)
    b, zb, _ = M.marginals(feats, [9, 4], trans, 1, dtype=torch.float32)
    assert b.dtype == torch.float32 and float((a - b.double()).abs().max()) < 1e-4 and float((za - zb.double()).abs().max()) < 1e-4


# ------------------------------------------------------------------------------------------------ the library, without a GPU
def test_symbol_is_declared_exported_and_bound():
    import os
    from multimodaltopicsegmentation_amd import _lib as L
    from multimodaltopicsegmentation_amd import ops
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'mts.h')).read()
    assert 'int mts_crf_marginals(' in header
    assert hasattr(L.lib, 'mts_crf_marginals') and len(L.SIGNATURES['mts_crf_marginals'][1]) == 11
    assert callable(ops.crf_marginals)


def test_bad_arguments_are_refused_before_any_device_work():
    from multimodaltopicsegmentation_amd import _lib as L
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)

    def call(B=1, Lq=2, C=4, cls=1, feats=p, trans=p, scores=p, ws=p):
        return L.lib.mts_crf_marginals(None, B, Lq, C, cls, feats, None, trans, scores, None, ws)

    for kw in (dict(C=2), dict(C=9), dict(C=4, cls=4), dict(C=5, cls=5), dict(cls=-1), dict(scores=None), dict(feats=None), dict(trans=None),
               dict(ws=None), dict(B=0), dict(Lq=0)):
        rc = call(**kw)
        assert rc == 1, kw                                             # MTS_ERR_INVALID
        with pytest.raises(ValueError, match='mts_crf_marginals'):
            L.check(rc)


# ------------------------------------------------------------------------------------------------ constructors and refusals
def test_birnncrf_decode_argument():
    from multimodaltopicsegmentation_amd import BiRnnCrf
    assert BiRnnCrf.DECODES == ('viterbi', 'marginal')
    plain = BiRnnCrf(2, 16, 8)
    assert plain.decode == 'viterbi' and plain.th is None
    marg = BiRnnCrf(2, 16, 8, decode='marginal')
    assert marg.decode == 'marginal' and marg.th is None
    assert list(marg.state_dict().keys()) == list(plain.state_dict().keys())          # decode is not state
    with pytest.raises(ValueError, match='decode'):
        BiRnnCrf(2, 16, 8, decode='posterior')
    with pytest.raises(ValueError, match='tagset_size'):
        BiRnnCrf(1, 16, 8, decode='marginal')
    assert BiRnnCrf(1, 16, 8).decode == 'viterbi'                      # the default mode keeps a single real tag


def test_textsegmenter_crf_decode_argument_and_the_sweep_refusal():
    from multimodaltopicsegmentation_amd import TextSegmenter
    from multimodaltopicsegmentation_amd.fit import _refusal
    with pytest.raises(ValueError, match='crf_decode'):
        TextSegmenter(2, 16, 8, architecture='biLSTMCRF', crf_decode='posterior')
    with pytest.raises(ValueError, match='biLSTMCRF'):
        TextSegmenter(2, 16, 8, architecture='BiLSTM', crf_decode='marginal')
    plain = TextSegmenter(2, 16, 8, architecture='biLSTMCRF', search_threshold=True)
    message = "search_threshold: architecture 'biLSTMCRF' decodes by Viterbi and has no decision threshold to search"
    assert plain.model.decode == 'viterbi' and plain._sweep_refusal() == message and plain._sweep is None
    assert _refusal(plain.model, 'Pk') == message
    marg = TextSegmenter(2, 16, 8, architecture='biLSTMCRF', crf_decode='marginal', search_threshold=True)
    assert marg.model.decode == 'marginal' and marg._sweep_refusal() is None and marg._sweep is not None
    assert _refusal(marg.model, 'Pk') is None and _refusal(marg.model, 'scaiano') is None
    assert 'segeval' in _refusal(marg.model, 'b')
