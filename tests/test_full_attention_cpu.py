"""CPU-only: Transformer_segmenter(restricted=False) -- the reference's full-attention (BertModel) tagger.

The fp64 restatement in tests/full_attention_oracle.py reproduces what the reference computed (tests/golden/g17_full_attention.npz,
written by tests/golden/make_golden_full_attention.py), and the tagger class accepts the reference's arguments and checkpoints.
"""
import numpy as np
import pytest
import torch

from tests.full_attention_oracle import full_attention, full_scores, tagger_loss
from tests.helpers import band_param_shapes, checksum, load, seeded_param

G17 = load('g17_full_attention')
CASES = ('a', 'b')


def case(k):
    g = {n[len(k) + 1:]: v for n, v in G17.items() if n.startswith(k + '_')}
    D, heads, ff, NL = (int(v) for v in g['cfg'])
    return g, D, heads, ff, NL


def params(D, ff, NL, n_out, seed):
    return {n: torch.from_numpy(seeded_param(n, s, seed)).double() for n, s in band_param_shapes(D, ff, NL, n_out).items()}


def loss_name(g):
    return 'FocalLoss' if g['scores'].shape[-1] == 1 else 'CrossEntropy'


@pytest.mark.parametrize('k', CASES)
def test_oracle_reproduces_the_reference(k):
    g, D, heads, ff, NL = case(k)
    n_out = g['scores'].shape[-1]
    p = params(D, ff, NL, n_out, int(g['seed']))
    for v in p.values():
        v.requires_grad_(True)
    x = torch.from_numpy(g['x']).double().requires_grad_(True)
    lengths = torch.from_numpy(g['lengths'])
    scores = full_scores(x, lengths, p, heads, NL)
    # every row, padded query rows included: the reference does not zero them, and they are not zero
    np.testing.assert_allclose(scores.detach().numpy(), g['scores'], rtol=1e-4, atol=2e-5)
    pad = torch.arange(g['x'].shape[1]).view(1, -1) >= lengths.view(-1, 1)
    assert pad.any() and float(scores.detach()[pad].abs().max()) > 1e-3
    loss = tagger_loss(scores, lengths, torch.from_numpy(g['tags']).double(), loss_name(g))
    assert abs(loss.item() - float(g['loss'])) < 1e-5 * max(1.0, abs(float(g['loss'])))
    loss.backward()
    np.testing.assert_allclose(x.grad.numpy(), g['gx'], rtol=1e-4, atol=1e-6)
    pe = 'model.model.embeddings.position_embeddings.weight'
    Lq = g['x'].shape[1]
    for n, v in p.items():
        gv = v.grad.numpy()
        if n == pe:
            assert not gv[Lq:].any()
            gv = gv[:Lq]
        if 'g.' + n in g:
            np.testing.assert_allclose(gv, g['g.' + n], rtol=1e-4, atol=1e-6, err_msg=n)
        else:
            np.testing.assert_allclose(checksum(gv), g['gsum.' + n], rtol=1e-4, atol=1e-6, err_msg=n)
            np.testing.assert_allclose(gv.ravel()[:32], g['ghead.' + n], rtol=1e-4, atol=1e-6, err_msg=n)


def test_full_attention_masks_padded_keys_only():
    torch.manual_seed(0)
    B, L, H, hd = 2, 9, 2, 4
    q, k, v = (torch.randn(B, L, H, hd, dtype=torch.float64) for _ in range(3))
    lengths = torch.tensor([9, 4])
    ctx, lse = full_attention(q, k, v, lengths, return_lse=True)
    k2, v2 = k.clone(), v.clone()
    k2[1, 4:] = 1e3
    v2[1, 4:] = -7.0                                   # padded keys / values of document 1 change nothing
    assert torch.equal(full_attention(q, k2, v2, lengths), ctx)
    s = torch.einsum('ihd,jhd->ihj', q[1], k[1, :4])
    assert torch.allclose(lse[1], torch.logsumexp(s, -1))


def test_constructs_on_cpu_with_the_reference_keys_and_loads_a_reference_state_dict():
    from multimodaltopicsegmentation_amd.taggers import Transformer_segmenter
    for k in CASES:
        g, D, heads, ff, NL = case(k)
        loss_fn = loss_name(g)
        m = Transformer_segmenter(2, D, ff, num_layers=NL, nheads=heads, loss_fn=loss_fn, restricted=False)
        assert not m.restricted and m.radii == [None] * NL
        sd = m.state_dict()
        assert set(sd) == set(str(s) for s in g['live_keys'])
        # positions 0..L-1 and no zeroed padding row (BERT's table)
        assert float(sd['model.model.embeddings.position_embeddings.weight'][1].abs().sum()) > 0
        if loss_fn == 'CrossEntropy':
            continue        # (the reference's CE tagger also carries its loss's class-weight buffer: the same for both attention paths)
        # a reference checkpoint: every key it has (HF's dead word embeddings, pooler, position_ids / token_type_ids buffers included)
        ref = {}
        shapes = band_param_shapes(D, ff, NL, 2 if loss_fn == 'CrossEntropy' else 1)
        for n in (str(s) for s in g['ref_keys']):
            ref[n] = torch.from_numpy(seeded_param(n, shapes[n], 5)) if n in shapes else torch.zeros(3)
        assert len(ref) > len(shapes)
        m.load_state_dict(ref, strict=True)
        got = m.state_dict()
        for n in shapes:
            assert torch.equal(got[n].float(), ref[n]), n


def test_window_size_is_ignored_and_odd_windows_are_accepted():
    from multimodaltopicsegmentation_amd.taggers import Transformer_segmenter
    with pytest.raises(AssertionError):
        Transformer_segmenter(2, 64, 32, num_layers=2, nheads=4, window_size=7)          # restricted: the reference's even-window assert
    m = Transformer_segmenter(2, 64, 32, num_layers=2, nheads=4, window_size=7, restricted=False)
    assert m.radii == [None, None]
    m = Transformer_segmenter(2, 64, 32, num_layers=3, nheads=4, window_size=127, dropout_out=0.3, restricted=False)
    assert m._attn_drop == 0.1 and m._pos_offset == 0                 # BertConfig's attention dropout; dropout_out is not used


def test_text_segmenter_reaches_the_full_attention_model():
    from multimodaltopicsegmentation_amd import TextSegmenter
    ts = TextSegmenter(2, 64, 32, num_layers=2, architecture='Transformer', loss_fn='FocalLoss', nheads=4, attention_window=7,
                       restricted=False)
    assert not ts.model.restricted and ts.model.radii == [None, None]
    ts = TextSegmenter(2, 64, 32, num_layers=2, architecture='Transformer', loss_fn='FocalLoss', nheads=4, attention_window=8)
    assert ts.model.restricted and ts.model.radii == [8, 4]
    assert ts.model._pos_offset == 2
