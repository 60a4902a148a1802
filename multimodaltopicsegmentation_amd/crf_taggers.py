"""Transformer-CRF: the restricted-window transformer encoder under the reference's CRF head (see taggers.py for the contract).

    TransformerCRF          models/CRF.py:481-506 composed with CRF (:98-240)

Upstream the class cannot be constructed (models/CRF.py:491) and its encoder would be the plain
``Transformer`` of NeuralArchitectures.py, which masks the valid sentences instead of the padding.  This one is built from the two pieces
that work and are pinned piece by piece: ``Transformer_segmenter``'s encoder (shared code, same parameters under the same state_dict
keys) and the ``CRF(embedding_dim, tagset_size)`` head of ``BiRnnCrf``.  DESIGN.md "Transformer-CRF tagger".

Training runs on PACKED rows like ``Transformer_segmenter``: the emissions come out of the last LayerNorm's fused head as
[n_valid, C] and the CRF kernels read them where they are (mts_crf_nll_packed), so nothing is unpacked for the loss and no gradient is
re-packed behind it.
"""
import torch

from . import _lib as L
from . import ops
from .taggers import _TaggerBase, _TransformerEncoderTagger, _linear_init

IMPOSSIBLE = -1e4


class TransformerCRF(_TransformerEncoderTagger):
    """Encoder of ``Transformer_segmenter`` (restricted=True: pyramidal local windows; restricted=False: full attention) -> fc(D -> tags + 2)
    fused into the last LayerNorm -> CRF NLL / Viterbi.  The reference's name and positional arguments; ``restricted``, ``window_size``,
    ``decode`` and ``compute_dtype`` are extensions.

    decode='marginal' (default 'viterbi'; DESIGN.md "CRF posterior-marginal decode"): ``forward`` scores every sentence with the logit of its
    posterior marginal P(y_t = 1 | x) and decodes by ``sigmoid(score) > th``, as ``BiRnnCrf(decode='marginal')``.  ``decode`` is not state.
    tagset_size 2 only (C = 4: the fused head covers four outputs)."""
    crf_head = True
    crf_architecture = 'Transformer-CRF'
    DECODES = ('viterbi', 'marginal')
    _HEAD_W, _HEAD_B = 'crf.fc.weight', 'crf.fc.bias'
    _GUARDED_ENTRY_POINTS = _TaggerBase._GUARDED_ENTRY_POINTS + ('marginal_scores',)

    def __init__(self, tagset_size, embedding_dim, hidden_dim, num_layers=6, nheads=8, dropout_in=0.0, dropout_out=0.0,
                 batch_first=True, positional_encoding=True, restricted=True, window_size=127, decode='viterbi', compute_dtype=None,
                 max_position_embedding=4096, seed=None):
        super().__init__()
        if decode not in self.DECODES:
            raise ValueError(f'decode must be one of {self.DECODES}, got {decode!r}')
        if tagset_size != 2:
            raise NotImplementedError(f'TransformerCRF supports tagset_size == 2 (C = 4 emissions per sentence), got {tagset_size}')
        self.decode = decode
        self._init_common('CrossEntropy', None, 0.9, 2, compute_dtype)
        self.num_tags = tagset_size + 2                       # models/CRF.py:108-110
        self.start_idx, self.stop_idx = self.num_tags - 2, self.num_tags - 1
        self._init_encoder(tagset_size, embedding_dim, hidden_dim, num_layers, nheads, dropout_in, dropout_out, restricted, window_size,
                           max_position_embedding, seed, self.num_tags)

    def _head_groups(self, gen, add):
        C, D = self.num_tags, self.embedding_dim
        fw, fb = _linear_init(C, D, gen)                      # CRF.fc = nn.Linear(in_features, num_tags), models/CRF.py:112
        trans = torch.randn(C, C, generator=gen)
        trans[self.start_idx, :] = IMPOSSIBLE                 # models/CRF.py:115-117
        trans[:, self.stop_idx] = IMPOSSIBLE
        g, t = [], []
        add(g, 'crf.fc.weight', (C, D), fw)
        add(g, 'crf.fc.bias', (C,), fb)
        add(t, 'crf.transitions', (C, C), trans)
        return [g, t]

    def _trans(self, flat):
        return self._w(flat, 'crf.transitions')

    # ---- public API ------------------------------------------------------------------------------------
    def loss_and_grad(self, xs, lengths, tags, want_grad=True):
        """Native forward(+backward): (loss 0-d fp32 tensor = mean over the documents of log Z - gold score, emissions [B, L, C] -- or
        [n_valid, C] when the batch was packed, see _pack_plan); gradients land in grad_flat."""
        L.require_gpu()
        x1, _, B, Lq, _ = self._split_input(xs)
        dev, C = x1.device, self.num_tags
        li32 = self._prep_lengths(lengths, B, Lq, dev)
        pack = self._pack_plan(lengths, B, Lq, dev)
        tg = tags.to(device=dev, dtype=torch.float32).contiguous()
        loss_out = torch.empty(2, dtype=torch.float32, device=dev)
        st = self._forward_native(xs, li32, pack=pack, need_hidden=False)
        N = st['N']
        g, lay = self.grad_flat(), self._layout
        dfe = self._ws.get('dfeats', N, C, torch.float32, dev) if want_grad else None
        dtr = lay.view(g, 'crf.transitions') if want_grad else None
        # the emissions where the fused head left them: packed rows addressed through row0, or the padded [B * L, C]
        ops.crf_nll_packed(st['scores'].view(N, C), tg, li32, self._trans(self._flat), loss_out, (B, Lq),
                           row0=pack['row0'] if pack else None, dfeats=dfe, dtrans=dtr)
        if want_grad:
            ops.scale_(dfe, self.loss_grad_scale)
            ops.scale_(dtr, self.loss_grad_scale)
            self._backward_native(st, dfe)                    # crf.fc.* from the head's passes; crf.transitions is final already
        return loss_out[0], st['scores']

    def loss(self, xs, lengths, tags):
        """models/CRF.py:495-499."""
        if torch.is_grad_enabled() and any(p.requires_grad for p in self._flat_params.values()):
            return self._autograd_loss(lambda: self.loss_and_grad(xs, lengths, tags, True)[0])
        return self.loss_and_grad(xs, lengths, tags, False)[0].clone()

    def _fwd(self, xs, lengths):
        x1, _, B, Lq, _ = self._split_input(xs)
        li32 = self._prep_lengths(lengths, B, Lq, x1.device)
        st = self._forward_native(xs, li32, need_hidden=False)           # inference keeps the padded layout
        return dict(B=B, L=Lq, li32=li32, feats=st['scores'])

    def _marginal_scores(self, st):
        B, Lq = st['B'], st['L']
        scores = torch.empty(B, Lq, 1, dtype=torch.float32, device=st['feats'].device)
        ops.crf_marginals(st['feats'], st['li32'], self._trans(self._flat), scores.view(B, Lq), cls=1)
        return scores

    def marginal_scores(self, xs, lengths):
        """-> [B, Lq, 1] fp32: the logit of P(y_t = 1 | x) clamped to +-80, 0 past a document's length (either decode mode)."""
        L.require_gpu()
        with torch.no_grad():
            return self._marginal_scores(self._fwd(xs, lengths))

    def forward(self, xs, lenghts, threshold=0.4):
        """models/CRF.py:501-506 -> (best_score [B], best_paths list of int lists).  decode='marginal': (scores [B, Lq, 1], list of
        per-document bool lists) by sigmoid(score) > th, ``.th`` over the argument, as Transformer_segmenter.forward."""
        L.require_gpu()
        with torch.no_grad():
            st = self._fwd(xs, lenghts)
            if self.decode == 'marginal':
                scores = self._marginal_scores(st)
                return scores, self._decode(scores, st['li32'], lenghts, threshold)
            B, Lq = st['B'], st['L']
            dev = st['feats'].device
            score = torch.empty(B, dtype=torch.float32, device=dev)
            paths = torch.empty(B, Lq, dtype=torch.int32, device=dev)
            ops.crf_viterbi(st['feats'], st['li32'], self._trans(self._flat), score, paths)
            ph = paths.cpu().numpy()
            L.check_async()
            lens = [int(v) for v in (lenghts.tolist() if lenghts is not None else [Lq] * B)]
        return score, [ph[i, :min(lens[i], Lq)].tolist() for i in range(B)]
