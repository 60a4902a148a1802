"""CPU: TransformerCRF's oracle against the reference-recorded pieces, the constructor and its state_dict, and the TextSegmenter
wiring of architecture='Transformer-CRF'.  No kernel runs here (tests/test_gpu_transformer_crf.py does that)."""
import numpy as np
import pytest
import torch

from tests import helpers as H
from tests import transformer_crf_oracle as O


def _t(a):
    return torch.from_numpy(np.asarray(a)).double()


def test_oracle_composition_reproduces_the_recorded_crf():
    """With the encoder's output replaced by g5's recorded features the composed oracle is the reference's CRF: its loss, its Viterbi
    score and every tag of its paths (the bounds of tests/test_oracle_vs_golden.py::test_crf_nll_and_viterbi)."""
    g = H.load('g5_crf')
    lengths = torch.from_numpy(g['lengths'])
    feats = _t(g['features'])
    p = {'crf.fc.weight': _t(g['fc.weight']), 'crf.fc.bias': _t(g['fc.bias']), 'crf.transitions': _t(g['transitions'])}
    loss = O.model_loss(None, lengths, _t(g['tags']), p, heads=1, num_layers=1, window=2, features=feats)
    assert abs(loss.item() - float(g['loss'])) < 1e-5
    score, paths = O.model_viterbi(None, lengths, p, heads=1, num_layers=1, window=2, features=feats)
    np.testing.assert_allclose(score.numpy(), g['viterbi_score'], rtol=1e-5)
    assert [v for p_ in paths for v in p_] == g['viterbi_paths'].tolist()
    assert [len(p_) for p_ in paths] == g['lengths'].tolist()
    # the path's own score, recomputed from the emissions, is the Viterbi score: path_score is what the bf16 GPU test measures with
    em = O.emissions(feats, p)
    for b, path in enumerate(paths):
        assert abs(float(O.path_score(em[b, :len(path)], path, p['crf.transitions'])) - float(score[b])) < 1e-9
    # the marginal logit's sign is a per-sentence decision of the same model: finite, clamped, 0 past the length
    logit = O.marginal_logits(feats, lengths, p)
    assert logit.shape == feats.shape[:2] and bool(torch.isfinite(logit).all()) and float(logit.abs().max()) <= 80.0
    for b, n in enumerate(lengths.tolist()):
        assert bool((logit[b, n:] == 0).all())


def test_constructor_state_dict_keys_and_shapes():
    from multimodaltopicsegmentation_amd import TransformerCRF, Transformer_segmenter
    D, F, NL = 32, 25, 2
    m = TransformerCRF(2, D, F, num_layers=NL, nheads=2, window_size=4, seed=5)
    sd = m.state_dict()
    ref = Transformer_segmenter(2, D, F, num_layers=NL, nheads=2, window_size=4, seed=5).state_dict()
    enc = [k for k in ref if not k.startswith('classification.')]
    assert [k for k in sd if not k.startswith('crf.')] == enc                      # the encoder: the same keys in the same order
    for k in enc:
        assert sd[k].shape == ref[k].shape and torch.equal(sd[k], ref[k]), k       # ... and, at one seed, the same initial values
    assert not any(k.startswith('classification.') for k in sd)
    assert sorted(k for k in sd if k.startswith('crf.')) == ['crf.fc.bias', 'crf.fc.weight', 'crf.transitions']
    assert sd['crf.fc.weight'].shape == (4, D) and sd['crf.fc.bias'].shape == (4,) and sd['crf.transitions'].shape == (4, 4)
    tr = sd['crf.transitions']
    assert bool((tr[2, :] == -1e4).all()) and bool((tr[:, 3] == -1e4).all())        # nothing enters START, nothing leaves STOP
    free = tr[[0, 1, 3]][:, [0, 1, 2]]
    assert bool((free.abs() < 10).all())
    assert m.num_tags == 4 and (m.start_idx, m.stop_idx) == (2, 3) and m.n_out == 4
    assert m.radii == [4, 2] and m.crf_head and m.decode == 'viterbi' and m.grad_hooks_cover_all is False
    assert TransformerCRF(2, D, F, num_layers=1, nheads=2, restricted=False).radii == [None]
    # a checkpoint round trip on the host
    m2 = TransformerCRF(2, D, F, num_layers=NL, nheads=2, window_size=4, seed=6)
    m2.load_state_dict(sd)
    assert all(torch.equal(v, m2.state_dict()[k]) for k, v in sd.items())


def test_constructor_argument_checks():
    from multimodaltopicsegmentation_amd import TransformerCRF
    with pytest.raises(ValueError, match='decode must be one of'):
        TransformerCRF(2, 32, 16, num_layers=1, nheads=2, window_size=4, decode='greedy')
    with pytest.raises(NotImplementedError, match='tagset_size == 2'):
        TransformerCRF(3, 32, 16, num_layers=1, nheads=2, window_size=4)
    with pytest.raises(ValueError, match='not a multiple of the number of attention heads'):
        TransformerCRF(2, 30, 16, num_layers=1, nheads=4, window_size=4)
    with pytest.raises(AssertionError, match='divisible by 2'):
        TransformerCRF(2, 32, 16, num_layers=1, nheads=2, window_size=127)          # the reference's own rule for the windows
    assert TransformerCRF(2, 32, 16, num_layers=1, nheads=2, window_size=4, decode='marginal').decode == 'marginal'


def test_text_segmenter_builds_the_architecture():
    from multimodaltopicsegmentation_amd import TextSegmenter, TransformerCRF
    from multimodaltopicsegmentation_amd import lightning_model as LM
    assert 'Transformer-CRF' not in LM._OUT_OF_SCOPE
    ts = TextSegmenter(2, 32, 16, num_layers=2, architecture='Transformer-CRF', nheads=2, attention_window=6, cosine_loss=True)
    assert isinstance(ts.model, TransformerCRF) and ts.cos is False and not ts.double_input and not ts.domain
    assert ts.model.radii == [6, 3] and ts.model.restricted and ts.model.decode == 'viterbi'
    assert any(k.startswith('model.crf.') for k in ts.state_dict())
    full = TextSegmenter(2, 32, 16, num_layers=1, architecture='Transformer-CRF', nheads=2, restricted=False, crf_decode='marginal')
    assert full.model.radii == [None] and full.model.decode == 'marginal'
    with pytest.raises(ValueError, match='crf_decode must be one of'):
        TextSegmenter(2, 32, 16, architecture='Transformer-CRF', nheads=2, attention_window=6, crf_decode='greedy')
    with pytest.raises(ValueError, match="crf_decode='marginal' applies to"):
        TextSegmenter(2, 32, 16, architecture='Transformer', nheads=2, attention_window=6, crf_decode='marginal')
    # the other refusals stay
    for arch in LM._OUT_OF_SCOPE:
        with pytest.raises(NotImplementedError):
            TextSegmenter(2, 32, 16, architecture=arch)
    with pytest.raises(ValueError, match='No other architectures'):
        TextSegmenter(2, 32, 16, architecture='Transformer-CRF2')


def test_viterbi_decode_is_refused_where_a_threshold_is_needed():
    """The places that ask "does this model decode by Viterbi?" answer for TransformerCRF as for BiRnnCrf: one shared predicate."""
    from multimodaltopicsegmentation_amd import BiRnnCrf, TextSegmenter, TransformerCRF
    from multimodaltopicsegmentation_amd.fit import _refusal
    from multimodaltopicsegmentation_amd.taggers import decodes_by_viterbi
    vit = TransformerCRF(2, 32, 16, num_layers=1, nheads=2, window_size=4)
    mar = TransformerCRF(2, 32, 16, num_layers=1, nheads=2, window_size=4, decode='marginal')
    assert decodes_by_viterbi(vit) and not decodes_by_viterbi(mar)
    assert decodes_by_viterbi(BiRnnCrf(2, 16, 8)) and not decodes_by_viterbi(BiRnnCrf(2, 16, 8, decode='marginal'))
    assert "'Transformer-CRF' decodes by Viterbi" in _refusal(vit, 'Pk') and _refusal(mar, 'Pk') is None
    assert "'biLSTMCRF' decodes by Viterbi" in _refusal(BiRnnCrf(2, 16, 8), 'Pk')
    ts = TextSegmenter(2, 32, 16, num_layers=1, architecture='Transformer-CRF', nheads=2, attention_window=4, search_threshold=True)
    assert "'Transformer-CRF' decodes by Viterbi" in ts._sweep_refusal() and ts._sweep is None
    with pytest.raises(NotImplementedError, match='decodes by Viterbi'):
        ts.on_validation_epoch_end()
    ts = TextSegmenter(2, 32, 16, num_layers=1, architecture='Transformer-CRF', nheads=2, attention_window=4, search_threshold=True,
                       crf_decode='marginal')
    assert ts._sweep_refusal() is None and ts._sweep is not None


def test_packed_entry_points_validate_before_any_launch():
    """MTS_ERR_INVALID (-> ValueError) for null operands, n_rows < 0 and C outside 3..8: argument checks come before any device work."""
    from multimodaltopicsegmentation_amd import _lib as L
    one = 1       # a non-null address that is never dereferenced: validation fails first
    for C in (2, 9):
        assert L.lib.mts_crf_nll_packed(None, 1, 1, C, one, one, 1, one, one, one, None, None, one, one, 1) == 1
        assert L.lib.mts_crf_viterbi_packed(None, 1, 1, C, one, one, one, one, one, one, one, 1) == 1
        assert L.lib.mts_crf_marginals_packed(None, 1, 1, C, 1, one, one, one, one, None, one, one, 1) == 1
    assert L.lib.mts_crf_nll_packed(None, 1, 1, 4, one, one, 1, one, one, one, None, None, one, one, -1) == 1
    assert L.lib.mts_crf_viterbi_packed(None, 1, 1, 4, one, one, one, one, one, one, one, -1) == 1
    assert L.lib.mts_crf_marginals_packed(None, 1, 1, 4, 1, one, one, one, one, None, one, one, -1) == 1
    assert L.lib.mts_crf_nll_packed(None, 1, 1, 4, None, one, 1, one, one, one, None, None, one, one, 1) == 1          # feats
    assert L.lib.mts_crf_nll_packed(None, 1, 1, 4, one, one, 1, one, one, one, None, one, one, one, 1) == 1           # dtrans without dfeats
    assert L.lib.mts_crf_nll_packed(None, 1, 1, 4, one, one, 1, None, one, one, None, None, one, one, 1) == 1          # row0 without lengths
    assert L.lib.mts_crf_viterbi_packed(None, 1, 1, 4, one, one, one, one, one, None, one, 1) == 1                     # bp_ws
    assert L.lib.mts_crf_marginals_packed(None, 1, 1, 4, 1, one, one, one, None, None, one, one, 1) == 1              # scores
    assert L.lib.mts_crf_marginals_packed(None, 1, 1, 4, 4, one, one, one, one, None, one, one, 1) == 1               # cls
    with pytest.raises(ValueError):
        L.check(1)
