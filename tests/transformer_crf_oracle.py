"""fp64 oracle of TransformerCRF: the encoder and the CRF of oracle.restatement, composed.

Upstream's ``TransformerCRF`` (models/CRF.py:481-506) cannot be constructed and its encoder is a dead path, so there
is no recorded output of the whole to compare with.  The two pieces are pinned on their own -- ``band_encoder`` by the fixtures of
``Transformer_segmenter`` (g3*), ``crf_nll`` / ``crf_viterbi`` by g5 -- and this module only wires one into the other:

    h = encoder(x)  ->  feats = h fc.weight^T + fc.bias  ->  mean_b(log Z_b - gold_b)  |  Viterbi  |  posterior marginals

``features=`` replaces the encoder's output, which is how tests/test_transformer_crf_cpu.py checks the wiring against g5.
Nothing of oracle/ is changed; the full-attention encoder and the marginals are the oracles the suite already has.
"""
import torch

from oracle import restatement as R
from tests.crf_marginal_oracle import clamped, marginals
from tests.full_attention_oracle import full_encoder


def encode(x, lengths, p, heads, num_layers, window, restricted=True):
    """[B, L, D] encoder output (every row, padded ones too), from a state_dict ``p`` of fp64 tensors"""
    if restricted:
        return R.band_encoder(x, lengths, p, heads, R.pyramidal_radii(num_layers, window))
    return full_encoder(x, lengths, p, heads, num_layers)


def _head(p):
    return p['crf.fc.weight'], p['crf.fc.bias'], p['crf.transitions']


def emissions(features, p):
    w, b, _ = _head(p)
    return features @ w.t() + b


def loss(features, lengths, tags, p):
    """``TransformerCRF.loss`` behind the encoder: mean over the documents of log Z - gold (models/CRF.py:495-499, :130-146)"""
    mask = R.create_mask(features.shape[1], lengths)
    return R.crf_nll(features, tags, mask, *_head(p))


def viterbi(features, lengths, p):
    """``TransformerCRF.forward`` behind the encoder -> (best_score [B], best_paths)"""
    mask = R.create_mask(features.shape[1], lengths)
    return R.crf_viterbi(features, mask, *_head(p))


def marginal_logits(features, lengths, p, cls=1):
    """decode='marginal': the clamped logit of P(y_t = cls | x) [B, L], 0 past each length"""
    logit, _, _ = marginals(emissions(features, p), [int(v) for v in lengths], p['crf.transitions'], cls)
    return clamped(logit)


def model_loss(x, lengths, tags, p, heads, num_layers, window, restricted=True, features=None):
    h = encode(x, lengths, p, heads, num_layers, window, restricted) if features is None else features
    return loss(h, lengths, tags, p)


def model_viterbi(x, lengths, p, heads, num_layers, window, restricted=True, features=None):
    h = encode(x, lengths, p, heads, num_layers, window, restricted) if features is None else features
    return viterbi(h, lengths, p)


def path_score(feats, path, trans):
    """score of one document's tag path under emissions feats [n, C] (fp64): sum_t T[y_t, y_{t-1}] + f_t(y_t), + T[stop, y_n]"""
    C = feats.shape[1]
    prev, s = C - 2, feats.new_zeros(())
    for t, y in enumerate(path):
        s = s + trans[y, prev] + feats[t, y]
        prev = y
    return s + trans[C - 1, prev]
