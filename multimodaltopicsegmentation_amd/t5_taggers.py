"""RecurrentLongT5 on the HIP kernels (reference: models/CRF.py:613-762, models/RestrictedTransformerLayer.py:135-187).

``num_layers`` identical blocks, each a 1-layer bidirectional ``RNN(embedding_dim, H)`` followed by a one-block LongT5 encoder on
width d = 2H as the reference's wrapper configures it: d_kv = 64 (inner = heads * 64), d_ff = 2H, ReLU feed-forward, no biases,
RMSNorm eps 1e-6, dropout_rate = dropout_in, relative_attention_num_buckets = max(4, r) and max distance r + 1 for the one-sided
radius r = window_size.  Then ``Linear(embedding_dim, 1)``, the BCE / focal loss and decode of the other taggers.

One block (drop = dropout(dropout_in), training mode only; the RNN's own two dropouts are always on):
    h = drop(x);  h = h + drop(o(attn(rms(h, w_ln0))));  h = h + drop(wo(drop(relu(wi(rms(h, w_ln1))))));  out = drop(rms(h, w_final))
attn: per head s_ij = q_i . k_j + T[bucket(j - i), h] over |j - i| <= r (include/mts.h, mts_t5_local_attn_fwd).
"""
import math

import torch

from . import _lib as L
from . import ops
from .flat import FlatLayout
from .rnn_taggers import _RnnStack, _RnnTaggerBase, _rnn_groups
from .taggers import _linear_init

D_KV = 64              # LongT5Config's d_kv: the wrapper never changes it
RMS_EPS = 1e-6         # LongT5Config's layer_norm_epsilon (the wrapper's layer_norm_eps=1e-12 is not passed on)
DEAD_KEYS = ('shared.weight', 'embed_tokens.weight')   # the token embedding of LongT5EncoderModel: never reached by inputs_embeds

_BUCKETS = {}


def num_buckets(radius):
    """relative_attention_num_buckets of the wrapper: max(4, window_size + 1 // 4) = max(4, r)."""
    return max(4, radius)


def relative_position_buckets(radius):
    """Bucket of each offset j - i = -r .. r ([2r + 1] int64), computed with the same torch ops as HF's bidirectional
    _relative_position_bucket (fp32 log) with num_buckets = max(4, r), max_distance = r + 1: bit-identical, and the kernels never
    evaluate the log."""
    nb = num_buckets(radius) // 2
    rp = torch.arange(-radius, radius + 1)
    ret = (rp > 0).to(torch.long) * nb
    rp = torch.abs(rp)
    me = nb // 2
    large = me + (torch.log(rp.float() / me) / math.log((radius + 1) / me) * (nb - me)).to(torch.long)
    large = torch.min(large, torch.full_like(large, nb - 1))
    return ret + torch.where(rp < me, rp, large)


def _bucket_table(radius, device):
    key = (radius, str(device))
    t = _BUCKETS.get(key)
    if t is None:
        t = _BUCKETS[key] = relative_position_buckets(radius).to(device=device, dtype=torch.int32)
    return t


class RecurrentLongT5(_RnnTaggerBase):
    """models/CRF.py:686-762."""
    grad_hooks_cover_all = False     # gradients are not announced span by span: NativeTrainer all-reduces after the backward

    def __init__(self, tagset_size, embedding_dim, hidden_dim, num_layers=6, nheads=8, dropout_in=0.0, dropout_out=0.0, batch_first=True,
                 loss_fn='CrossEntropy', threshold=None, window_size=127, alpha=0.9, gamma=2, compute_dtype=None, seed=None):
        super().__init__()
        if loss_fn == 'CrossEntropy':
            # models/CRF.py:702 reads self.tagset_size, which the reference never sets
            raise AttributeError("'RecurrentLongT5' object has no attribute 'tagset_size'")
        self._init_common(loss_fn, threshold, alpha, gamma, compute_dtype)
        self._check_rnn_args(dropout_in, dropout_out, True, True)
        if hidden_dim % 8:
            raise NotImplementedError(f'RecurrentLongT5: hidden_dim={hidden_dim} must be a multiple of 8 (the LongT5 width 2H is not '
                                      'stored padded)')
        if not 1 <= int(window_size) <= 1024:
            raise NotImplementedError(f'RecurrentLongT5: window_size={window_size} outside the local-attention kernels\' 1..1024')
        self.embedding_dim, self.hidden_dim, self.num_layers, self.nheads = embedding_dim, hidden_dim, num_layers, nheads
        self.radius = int(window_size)
        self.n_buckets = num_buckets(self.radius)
        self.n_out = 1
        d, inner = 2 * hidden_dim, nheads * D_KV
        self._d, self._inner = d, inner
        gen = torch.Generator().manual_seed(torch.initial_seed() if seed is None else seed)
        groups, init, pads = [], {}, {}
        self._names = []
        for k in range(num_layers):
            g, i, p = _rnn_groups(f'model.{k}.lstm.', embedding_dim, hidden_dim, 1, gen)
            groups += g
            init.update(i)
            pads.update(p)
            tp = f'model.{k}.transformer.model.encoder.'
            a = tp + 'block.0.layer.0.LocalSelfAttention.'
            f = tp + 'block.0.layer.1.'
            n = dict(q=a + 'q.weight', k=a + 'k.weight', v=a + 'v.weight', o=a + 'o.weight', rel=a + 'relative_attention_bias.weight',
                     ln0=tp + 'block.0.layer.0.layer_norm.weight', wi=f + 'DenseReluDense.wi.weight', wo=f + 'DenseReluDense.wo.weight',
                     ln1=f + 'layer_norm.weight', fin=tp + 'final_layer_norm.weight')
            self._names.append(n)
            # HF LongT5PreTrainedModel._init_weights (factor 1): normal with std d^-0.5 (q: (d d_kv)^-0.5, o: inner^-0.5, wo: d_ff^-0.5)
            shapes = dict(q=(inner, d), k=(inner, d), v=(inner, d), o=(d, inner), rel=(self.n_buckets, nheads), ln0=(d,), wi=(d, d),
                          wo=(d, d), ln1=(d,), fin=(d,))
            std = dict(q=(d * D_KV) ** -0.5, k=d ** -0.5, v=d ** -0.5, o=inner ** -0.5, rel=d ** -0.5, wi=d ** -0.5, wo=d ** -0.5)
            for grp in (('q', 'k', 'v'), ('o',), ('rel',), ('ln0', 'ln1', 'fin'), ('wi',), ('wo',)):
                groups.append([(n[s], shapes[s]) for s in grp])
                for s in grp:
                    init[n[s]] = torch.ones(shapes[s]) if s in ('ln0', 'ln1', 'fin') else torch.randn(shapes[s], generator=gen) * std[s]
        cw, cb = _linear_init(1, embedding_dim, gen)
        groups.append([('classification.weight', (1, embedding_dim)), ('classification.bias', (1,))])
        init['classification.weight'], init['classification.bias'] = cw, cb
        self._init_flat(FlatLayout(groups, pads), init)
        self._rnns = [_RnnStack(self, f'model.{k}.lstm.', embedding_dim, hidden_dim, 1, f'lt{k}') for k in range(num_layers)]
        self._register_load_state_dict_pre_hook(self._drop_dead_keys)

    @staticmethod
    def _drop_dead_keys(state_dict, prefix, *args):
        """A reference checkpoint carries LongT5EncoderModel's token embedding (shared.weight, [32128, d], and its alias
        encoder.embed_tokens.weight) per block; inputs_embeds never reaches it: ignore it on load."""
        for k in [k for k in state_dict if k.startswith(prefix) and k.endswith(DEAD_KEYS)]:
            del state_dict[k]

    # ---- helpers ---------------------------------------------------------------------------------
    def _mat(self, flat, name, rows, cols):
        return self._wspan(flat, name, name, rows, cols)

    def _check_width(self, xs, lengths):
        """Called first by every entry point, so the reference's error comes before anything else (a missing GPU included)."""
        if self.embedding_dim != 2 * self.hidden_dim:
            B = xs.shape[0]
            Lq = min(int(lengths.max()), xs.shape[1]) if lengths is not None else xs.shape[1]
            # the reference builds every block's RNN with embedding_dim inputs and the head with embedding_dim: the first call fails
            # in the head's matmul (one block) or in block 2's LSTM (more)
            H2 = 2 * self.hidden_dim
            if self.num_layers == 1:
                raise RuntimeError(f'mat1 and mat2 shapes cannot be multiplied ({B * Lq}x{H2} and {self.embedding_dim}x1)')
            n = int(lengths.sum()) if lengths is not None else B * Lq
            raise RuntimeError(f'mat1 and mat2 shapes cannot be multiplied ({n}x{H2} and {self.embedding_dim}x{4 * self.hidden_dim})')

    def _dropout(self, x, p, tag, keep_mask):
        """y = dropout(x) into a workspace buffer; (y, mask or None)."""
        y = self._ws.get('dr_' + tag, x.shape[0], x.shape[1], x.dtype, x.device)
        mask = self._ws.get('dm_' + tag, x.shape[0], x.shape[1], torch.uint8, x.device) if keep_mask else None
        ops.dropout_fwd(x, y, p, self._drop_seed(), mask=mask)
        return y, mask

    # ---- forward -----------------------------------------------------------------------------------
    def _block_fwd(self, k, xin, li32, B, Lq, want_grad):
        n, dt, dev = self._names[k], self.compute_dtype, xin.device
        N, d, inner, heads, r = B * Lq, self._d, self._inner, self.nheads, self.radius
        wf, pf = self._weights(), self._flat
        ws = lambda name, cols, dtype=dt: self._ws.get(f'b{k}{name}', N, cols, dtype, dev)   # noqa: E731
        p = self.dropout_in if self.training else 0.0          # the T5 layer's dropouts follow train / eval
        S = dict(inmask=None)
        if self.dropout_in:                                    # RNN input dropout (always on); blocks above the first need its mask
            xin, S['inmask'] = self._dropout(xin, self.dropout_in, f'b{k}in', want_grad and k > 0)
        hl, S['saved'] = self._rnns[k].forward(xin, li32, B, Lq)
        S['hmask'] = None
        if self.dropout_out:
            hl, S['hmask'] = self._dropout(hl, self.dropout_out, f'b{k}out', want_grad)
        h0, S['m0'] = (self._dropout(hl, p, f'b{k}m0', want_grad) if p else (hl, None))
        a, r0 = ws('a', d), ws('r0', 1, torch.float32)
        ops.rmsnorm_fwd(h0, self._w(pf, n['ln0']), RMS_EPS, a, r0)
        qkv = ws('qkv', 3 * inner)
        ops.linear_fwd(a, self._wspan(wf, n['q'], n['v'], 3 * inner, d), None, qkv)
        ctx, lse = ws('ctx', inner), ws('lse', heads, torch.float32)
        S['attn_seed'] = self._drop_seed() if p else 0
        ops.t5_local_attn_fwd(qkv, li32, B, Lq, heads, r, self._w(pf, n['rel']), _bucket_table(r, dev), ctx, lse, p, S['attn_seed'])
        h1 = ws('h1', d)
        wo_att = self._mat(wf, n['o'], d, inner)
        S['m1'] = None
        if p:
            t = ws('t1', d)
            ops.linear_fwd(ctx, wo_att, None, t)
            S['m1'] = ws('m1', d, torch.uint8)
            ops.dropout_fwd(t, h1, p, self._drop_seed(), mask=S['m1'], residual=h0)
        else:
            ops.linear_fwd(ctx, wo_att, None, h1, residual=h0)
        bn, r1 = ws('bn', d), ws('r1', 1, torch.float32)
        ops.rmsnorm_fwd(h1, self._w(pf, n['ln1']), RMS_EPS, bn, r1)
        u, f = ws('u', d), ws('f', d)
        ops.linear_fwd(bn, self._mat(wf, n['wi'], d, d), None, f, relu=True, aux=u)
        S['m2'] = None
        if p:
            f, S['m2'] = self._dropout(f, p, f'b{k}m2', want_grad)
        h2 = ws('h2', d)
        wo_ff = self._mat(wf, n['wo'], d, d)
        S['m3'] = None
        if p:
            t = ws('t2', d)
            ops.linear_fwd(f, wo_ff, None, t)
            S['m3'] = ws('m3', d, torch.uint8)
            ops.dropout_fwd(t, h2, p, self._drop_seed(), mask=S['m3'], residual=h1)
        else:
            ops.linear_fwd(f, wo_ff, None, h2, residual=h1)
        out, r2 = ws('out', d), ws('r2', 1, torch.float32)
        ops.rmsnorm_fwd(h2, self._w(pf, n['fin']), RMS_EPS, out, r2)
        S['m4'] = None
        if p:
            out, S['m4'] = self._dropout(out, p, f'b{k}m4', want_grad)
        S.update(p=p, h0=h0, a=a, r0=r0, qkv=qkv, ctx=ctx, lse=lse, h1=h1, bn=bn, r1=r1, u=u, f=f, h2=h2, r2=r2)
        return out, S

    def _fwd(self, xs, lengths, want_grad):
        x, Lq = self._prep_input(xs, lengths)
        B, dev = x.shape[0], x.device
        li32 = self._prep_lengths(lengths, B, Lq, dev)
        h = self._to_act(x)
        blocks = []
        for k in range(self.num_layers):
            h, S = self._block_fwd(k, h, li32, B, Lq, want_grad)
            blocks.append(S)
        scores = self._ws.get('scores', B * Lq, 1, torch.float32, dev)
        ops.head_fwd(h, self._w(self._flat, 'classification.weight'), self._w(self._flat, 'classification.bias'), scores)
        return dict(B=B, L=Lq, li32=li32, h=h, blocks=blocks, scores=scores.view(B, Lq, 1))

    # ---- backward ----------------------------------------------------------------------------------
    def _block_bwd(self, k, S, dout, li32, B, Lq):
        n, dt, dev = self._names[k], self.compute_dtype, dout.device
        N, d, inner, heads, r, p = B * Lq, self._d, self._inner, self.nheads, self.radius, S['p']
        wf, pf, g, lay = self._weights(), self._flat, self.grad_flat(), self._layout
        ws = lambda name, cols: self._ws.get(f'b{k}{name}', N, cols, dt, dev)   # noqa: E731
        gv = lambda name: lay.view(g, name)                                    # noqa: E731
        if S['m4'] is not None:
            ops.dropout_bwd(dout, dout, S['m4'], p)
        dh = ws('dh', d)                                       # the residual stream's gradient, accumulated in place
        ops.rmsnorm_bwd(S['h2'], dout, self._w(pf, n['fin']), S['r2'], dh, gv(n['fin']))
        dy = dh
        if S['m3'] is not None:
            dy = ws('dy', d)
            ops.dropout_bwd(dh, dy, S['m3'], p)
        ops.linear_wgrad(dy, S['f'], gv(n['wo']))
        df = ws('df', d)
        ops.linear_dgrad(dy, self._mat(wf, n['wo'], d, d), df)
        if S['m2'] is not None:
            ops.dropout_bwd(df, df, S['m2'], p)
        ops.relu_bwd(S['u'], df)
        ops.linear_wgrad(df, S['bn'], gv(n['wi']))
        db = ws('db', d)
        ops.linear_dgrad(df, self._mat(wf, n['wi'], d, d), db)
        ops.rmsnorm_bwd(S['h1'], db, self._w(pf, n['ln1']), S['r1'], dh, gv(n['ln1']), dres=dh)
        dy = dh
        if S['m1'] is not None:
            dy = ws('dy', d)
            ops.dropout_bwd(dh, dy, S['m1'], p)
        ops.linear_wgrad(dy, S['ctx'], gv(n['o']))
        dctx = ws('dctx', inner)
        ops.linear_dgrad(dy, self._mat(wf, n['o'], d, inner), dctx)
        dqkv = ws('dqkv', 3 * inner)
        ops.t5_local_attn_bwd(S['qkv'], li32, B, Lq, heads, r, self._w(pf, n['rel']), _bucket_table(r, dev), S['lse'], S['ctx'], dctx,
                              dqkv, gv(n['rel']), p, S['attn_seed'])
        off, cnt = lay.span(n['q'], n['v'])
        ops.linear_wgrad(dqkv, S['a'], g[off:off + cnt].view(3 * inner, d))
        da = ws('da', d)
        ops.linear_dgrad(dqkv, self._wspan(wf, n['q'], n['v'], 3 * inner, d), da)
        ops.rmsnorm_bwd(S['h0'], da, self._w(pf, n['ln0']), S['r0'], dh, gv(n['ln0']), dres=dh)
        if S['m0'] is not None:
            ops.dropout_bwd(dh, dh, S['m0'], p)
        if S['hmask'] is not None:
            ops.dropout_bwd(dh, dh, S['hmask'], self.dropout_out)
        rnn = self._rnns[k]
        rnn.backward(S['saved'], dh, li32, B, Lq)
        if k == 0:
            return None
        H8, D = 8 * rnn.H, rnn.D
        dxproj = self._ws.get(f'{rnn.tag}dxproj0', N, H8, dt, dev)             # left by rnn.backward
        dprev = self._ws.get(f'b{k}dprev', N, D, dt, dev)
        ops.linear_dgrad(dxproj, self._wspan(wf, *rnn._names('weight_ih', 0), H8, D), dprev)
        if S['inmask'] is not None:
            ops.dropout_bwd(dprev, dprev, S['inmask'], self.dropout_in)
        return dprev

    def loss_and_grad(self, xs, lengths, tags, want_grad=True):
        self._check_width(xs, lengths)
        L.require_gpu()
        st = self._fwd(xs, lengths, want_grad)
        dev, B, Lq = st['scores'].device, st['B'], st['L']
        tg = tags.to(device=dev, dtype=torch.float32).contiguous()
        loss_out = torch.empty(2, dtype=torch.float32, device=dev)
        dsc = self._ws.get('dscores', B * Lq, 1, torch.float32, dev) if want_grad else None
        ops.tagger_loss(self.loss_kind, st['scores'], tg, st['li32'], self.alpha, self.gamma, loss_out, dsc)
        if want_grad:
            ops.scale_(dsc, self.loss_grad_scale)
            g, lay = self.grad_flat(), self._layout
            ops.head_bwd_params(st['h'], dsc, lay.view(g, 'classification.weight'), lay.view(g, 'classification.bias'))
            dout = self._ws.get('dout', B * Lq, self.embedding_dim, self.compute_dtype, dev)
            ops.head_bwd_data(dsc, self._w(self._flat, 'classification.weight'), dout)
            for k in range(self.num_layers - 1, -1, -1):
                dout = self._block_bwd(k, st['blocks'][k], dout, st['li32'], B, Lq)
        return loss_out[0], st['scores']

    def loss(self, xs, lengths, tags, segments=None):
        """models/CRF.py:722-745."""
        if segments is not None:
            raise NotImplementedError('cosine auxiliary loss (models/CRF.py:23-92): no collater of the reference produces '
                                      "batch['src_segments'] (TextSegmenter.training_step raises KeyError upstream, fixture g15)")
        if torch.is_grad_enabled() and any(p.requires_grad for p in self._flat_params.values()):
            return self._autograd_loss(lambda: self.loss_and_grad(xs, lengths, tags, True)[0])
        return self.loss_and_grad(xs, lengths, tags, False)[0].clone()

    def forward(self, xs, lenghts, threshold=0.4):
        """models/CRF.py:747-762: scores [B, max(len), 1] (padded rows included) and tag lists trimmed to each length."""
        self._check_width(xs, lenghts)
        L.require_gpu()
        with torch.no_grad():
            st = self._fwd(xs, lenghts, False)
            scores = st['scores'].clone()
            tags = self._decode(scores, st['li32'], lenghts, threshold)
        return scores, tags
