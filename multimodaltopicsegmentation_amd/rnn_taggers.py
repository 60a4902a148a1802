"""Recurrent taggers on the HIP kernels: BiLSTM, BiLSTMLateFusion, BiRnnCrf (see taggers.py for the contract).

Reference: models/NeuralArchitectures.py:23-145 (RNN), models/CRF.py:274-369 (BiLSTM), :371-479 (BiLSTMLateFusion),
:243-272 + :98-240 (BiRnnCrf + CRF; the reference wrapper unpacks a single tensor and crashes, SURVEY.md Q2 -- this
one composes RNN -> CRF the way the reference evidently intended).
"""
import math
import os

import torch
import torch.nn as nn

from . import _lib as L
from . import ops
from .flat import FlatLayout, round_up
from .taggers import _TaggerBase, _linear_init, _xavier_uniform, LOSS_KINDS

IMPOSSIBLE = -1e4   # models/CRF.py:95


def _rnn_groups(prefix, D, H, num_layers, gen):
    """Parameter groups + Keras-style init of ``RNN._reinitialize`` (NeuralArchitectures.py:58-79): xavier_uniform
    W_ih, orthogonal W_hh, zero biases with the forget-gate slice of bias_ih set to 1.  The two directions of a
    layer are adjacent so that one [8H, Din] GEMM projects both.

    Returns (groups of STORAGE shapes, init values in the reference's shapes, pad specs): hidden size and input width are
    stored rounded up to a multiple of 8 (the reference's default hidden size is 25); see flat.py "padded storage"."""
    Hp, Dp = round_up(H, 8), round_up(D, 8)
    groups, init, pads = [], {}, {}
    gate_rows = [(0, 4, H, Hp)] if Hp != H else []
    for k in range(num_layers):
        din, din_p = (D, Dp) if k == 0 else (2 * H, 2 * Hp)
        col = ([(1, 1, D, Dp)] if Dp != D else []) if k == 0 else ([(1, 2, H, Hp)] if Hp != H else [])
        g = []
        for sfx in ('', '_reverse'):
            n = f'{prefix}rnn.weight_ih_l{k}{sfx}'
            g.append((n, (4 * Hp, din_p)))
            init[n] = _xavier_uniform((4 * H, din), gen)
            if gate_rows or col:
                pads[n] = gate_rows + col
        groups.append(g)
        g = []
        for sfx in ('', '_reverse'):
            n = f'{prefix}rnn.weight_hh_l{k}{sfx}'
            g.append((n, (4 * Hp, Hp)))
            w = torch.empty(4 * H, H)
            nn.init.orthogonal_(w, generator=gen)
            init[n] = w
            if gate_rows:
                pads[n] = gate_rows + [(1, 1, H, Hp)]
        groups.append(g)
        for kind in ('bias_ih', 'bias_hh'):
            g = []
            for sfx in ('', '_reverse'):
                n = f'{prefix}rnn.{kind}_l{k}{sfx}'
                g.append((n, (4 * Hp,)))
                b = torch.zeros(4 * H)
                if kind == 'bias_ih':
                    b[H:2 * H] = 1.0
                init[n] = b
                if gate_rows:
                    pads[n] = gate_rows
            groups.append(g)
    return groups, init, pads


def _head_pad(H, nblocks):
    """Pad spec of a head weight [n_out, nblocks*H] reading nblocks concatenated hidden vectors."""
    Hp = round_up(H, 8)
    return [(1, nblocks, H, Hp)] if Hp != H else None


class _RnnStack:
    """Native forward/backward of one ``RNN`` (bidirectional multi-layer LSTM) living inside a flat-parameter model."""

    def __init__(self, owner, prefix, D, H, num_layers, tag):
        """D, H: the reference's sizes; the kernels run on the padded ones (multiples of 8, padded units inert)."""
        self.o, self.prefix, self.D, self.H, self.nl, self.tag = owner, prefix, round_up(D, 8), round_up(H, 8), num_layers, tag

    def _names(self, kind, k):
        return f'{self.prefix}rnn.{kind}_l{k}', f'{self.prefix}rnn.{kind}_l{k}_reverse'

    def forward(self, x2d, lengths_i32, B, Lq):
        """x2d: [B*Lq, D] in compute dtype.  Returns (out [N, 2H], saved state)."""
        o, H = self.o, self.H
        dt, dev = o.compute_dtype, x2d.device
        N = B * Lq
        wf, pf = o._weights(), o._flat
        saved = []
        h = x2d
        for k in range(self.nl):
            din = h.shape[1]
            w_ih = o._wspan(wf, *self._names('weight_ih', k), 8 * H, din)
            b_ih = o._wspan(pf, *self._names('bias_ih', k), 1, 8 * H).view(-1)
            b_hh = o._wspan(pf, *self._names('bias_hh', k), 1, 8 * H).view(-1)
            w_hh = o._wspan(pf, *self._names('weight_hh', k), 8 * H, H)
            xproj = o._ws.get(f'{self.tag}xproj{k}', N, 8 * H, dt, dev)
            ops.linear_fwd(h, w_ih, b_ih, xproj)
            out = o._ws.get(f'{self.tag}out{k}', N, 2 * H, dt, dev)
            gates = o._ws.get(f'{self.tag}gates{k}', N, 8 * H, dt, dev)
            cells = o._ws.get(f'{self.tag}cells{k}', N, 2 * H, torch.float32, dev)
            ops.lstm_fwd(xproj, w_hh, b_hh, lengths_i32, B, Lq, H, 2, out, gates, cells)
            saved.append(dict(hin=h, out=out, gates=gates, cells=cells))
            h = out
        return h, saved

    overlap_wgrad = True     # every layer's parameter gradients on side streams, off the chain of dependent launches: the recurrence occupies
                             # 32 of the 256 CUs and is pure dependent-step latency, and what follows it on the critical path is ONE data-
                             # gradient GEMM -- h_{t-1} + dW_hh (two split-K GEMMs and their reduces, ~80 us per layer at 64 x 256, H = 256) and
                             # the bias sums + dW_ih (~140 us) wait for nobody until the optimizer.  Round 3 kept dW_hh behind every recurrence
                             # on the main stream (inside mts_lstm_bwd) and ran layer 0's gradients, all of them, after its recurrence, one
                             # after the other (mts_lstm_bwd_recurrence / _whh split the call; which arrangement: overlap_mode below)

    # Measured, one box per table (profiles/r04_rnn_overlap_modes.txt; ms per step, BiLSTM 64 x 256 | late fusion 64 x 512):
    #   0 everything on the issuing stream                                            3.087 | 7.24
    #   1 both chains (h_{t-1} + dW_hh, then bias sums + dW_ih) on ONE side stream    3.014 | 7.07      <- default
    #   2 the two chains on two side streams                                          3.020 | 8.0 (its two extra streams crowd the hardware queues)
    #   3 dW_hh on the issuing stream behind the data gradient, the rest on a side stream   3.068 | 7.21
    #   4 as 3, layers above the first only; 5 round 3 call for call (h_{t-1} in front of the recurrence, dW_hh behind it, on the issuing stream)   3.087 | 7.24, 7.20
    # The chains do not come for free: next to a recurrence the 128-tile dW_hh GEMMs take 61 us instead of 25 and the recurrence 663 us instead
    # of 639 (rocprofv3 of modes 0 / 2) -- both poll / stream through the same L2s.
    overlap_mode = None if os.environ.get('MTS_RNN_OVERLAP') is None else int(os.environ['MTS_RNN_OVERLAP'])

    def _wg_streams(self, dev, n):
        """n (1 | 2) of the small shared pool of side streams for this encoder: the dW_hh chain's and the bias + dW_ih chain's (late fusion: pool
        stream 0 is the second encoder's own).  Only the streams a mode USES are created: HIP hands its hardware queues out in creation order, and
        two unused streams of the pool in front of the ones that matter moved late fusion's encoders onto one queue (8.2 against 7.2 ms)."""
        base = 2 if self.tag == 'r2' else 1
        return tuple(ops.side_stream(dev, base + 2 * i) for i in range(n))

    def backward(self, saved, dout, lengths_i32, B, Lq):
        o, H = self.o, self.H
        dt, dev = o.compute_dtype, dout.device
        N = B * Lq
        wf, pf, lay = o._weights(), o._flat, o._layout
        g = o.grad_flat()
        cur = torch.cuda.current_stream(dev) if dev.type == 'cuda' else None
        # not under a data-parallel hook: with RCCL's streams and late fusion's second encoder stream in the process two more streams
        # made the step slower, not faster (one-rank RCCL run at 64 x 512: 8.69 ms against 7.75 without them; 7.56 / 7.74 without a hook)
        mode = self.overlap_mode if self.overlap_mode is not None else 1
        if not (self.overlap_wgrad and o._grad_hook is None and cur is not None) or (mode == 4 and self.nl < 2):
            mode = 0
        sides = self._wg_streams(dev, 2 if mode == 2 else 1) if mode else None
        for k in range(self.nl - 1, -1, -1):
            S = saved[k]
            din = S['hin'].shape[1]
            w_hh = o._wspan(pf, *self._names('weight_hh', k), 8 * H, H)
            # one buffer PER LAYER: layer k's weight gradient and bias sums read its dxproj on the side streams, and nothing on the main
            # stream waits for them before the loop ends -- a buffer shared by layers k and k - 2 (two buffers, as this was) is rewritten by
            # layer k - 2's recurrence with only "a recurrence outlasts a GEMM" in between (silent corruption at >= 3 layers)
            dxproj = o._ws.get(f'{self.tag}dxproj{k}', N, 8 * H, dt, dev)
            # ... and one recurrence workspace per layer: mts_lstm_bwd_whh finds (or builds) h_{t-1} in it and takes its split-K slabs from it
            # while the next layer's recurrence is already running
            ws = ops.lstm_workspace(dt, B, Lq, H, 2, dev, tag=f'{self.tag}lstm{k}')
            off_hh, n_hh = lay.span(*self._names('weight_hh', k))
            if mode == 5:                              # round 3, call for call: h_{t-1}, recurrence, dW_hh in ONE call on the issuing stream
                ops.lstm_bwd(w_hh, lengths_i32, S['out'], S['gates'], S['cells'], dout, B, Lq, H, 2, dxproj, g[off_hh:off_hh + n_hh], ws=ws)
            else:
                ops.lstm_bwd_recurrence(w_hh, lengths_i32, S['out'], S['gates'], S['cells'], dout, B, Lq, H, 2, dxproj, ws)
            ev = None
            if sides is not None:
                ev = torch.cuda.Event()
                ev.record(cur)                         # dxproj of layer k is complete on the issuing stream
            if k > 0:                                  # the critical path first: what the next recurrence needs
                dprev = o._ws.get(f'{self.tag}dprev{k & 1}', N, din, dt, dev)
                ops.linear_dgrad(dxproj, o._wspan(wf, *self._names('weight_ih', k), 8 * H, din), dprev)
                dout = dprev

            def whh_of_layer():
                ops.lstm_bwd_whh(lengths_i32, S['out'], dxproj, B, Lq, H, 2, g[off_hh:off_hh + n_hh], ws)

            def params_of_layer():
                off, n = lay.span(*self._names('bias_ih', k))
                ops.colsum(dxproj, g[off:off + n])
                off2, n2 = lay.span(*self._names('bias_hh', k))
                g[off2:off2 + n2].copy_(g[off:off + n])
                off, n = lay.span(*self._names('weight_ih', k))
                ops.linear_wgrad(dxproj, S['hin'], g[off:off + n].view(8 * H, din))

            if mode == 2:                              # two chains, two streams
                for side, fn in zip(sides, (whh_of_layer, params_of_layer)):
                    side.wait_event(ev)
                    with torch.cuda.stream(side):
                        fn()
            elif mode == 1:                            # one side stream, both chains one after the other
                sides[0].wait_event(ev)
                with torch.cuda.stream(sides[0]):
                    whh_of_layer()
                    params_of_layer()
            elif mode == 5:
                if k > 0:
                    sides[0].wait_event(ev)
                    with torch.cuda.stream(sides[0]):
                        params_of_layer()
                else:
                    params_of_layer()
            elif mode == 3 or (mode == 4 and k > 0):   # dW_hh behind the data gradient on the main stream, the rest on a side stream
                whh_of_layer()                         # (4: only for the layers above the first -- round 3's arrangement)
                sides[0].wait_event(ev)
                with torch.cuda.stream(sides[0]):
                    params_of_layer()
            else:
                whh_of_layer()
                params_of_layer()
                # layer k's parameters (both directions: W_ih, W_hh, b_ih, b_hh are adjacent groups) are final: a data-parallel
                # trainer may start reducing them while the lower layers' recurrences still run (announced from the stream that
                # produced them: the collective is ordered behind it)
                a0 = lay.entries[self._names('weight_ih', k)[0]][0]
                b0, bn = lay.span(*self._names('bias_hh', k))
                o._grads_ready(a0, b0 + bn)
        if sides is not None:
            for side in sides:
                cur.wait_stream(side)                  # every gradient has landed before the caller (optimizer, exchange waits) goes on


class _RnnTaggerBase(_TaggerBase):
    grad_hooks_cover_all = True      # every parameter span is announced through _grads_ready (trainer.NativeTrainer overlaps the exchange)

    def _span_of(self, first, last):
        a, _ = self._layout.entries[first]
        b, n = self._layout.span(last, last)
        return a, b + n

    def _check_rnn_args(self, dropout_in, dropout_out, LSTM, bidirectional):
        for pr in (dropout_in, dropout_out):
            if not 0.0 <= float(pr) < 1.0:
                raise ValueError(f'dropout probability has to be between 0 and 1, but got {pr}')      # F.dropout's own check
        # RNN.forward calls F.dropout(x, p) WITHOUT training=..., so the reference drops in eval mode too; same here
        self.dropout_in, self.dropout_out = float(dropout_in), float(dropout_out)
        self._drop_calls = 0
        if not LSTM:
            # dead upstream (fixture tests/golden/g15_adjacent_encoders.npz): RNN.forward hands nn.GRU an (h0, c0) tuple
            # (NeuralArchitectures.py:104-113) -> AttributeError: 'tuple' object has no attribute 'index_select' on every call
            raise NotImplementedError('GRU (LSTM=False, NeuralArchitectures.py:46-50): the reference itself raises AttributeError on '
                                      'every tagger call with this option; there is no behaviour to reproduce')
        if not bidirectional:
            # dead upstream (g15): :134-145 returns the PackedSequence un-padded -> TypeError in the tagger's nn.Linear
            raise NotImplementedError('unidirectional RNN (bidirectional=False, NeuralArchitectures.py:134-145): the reference itself '
                                      'raises TypeError (PackedSequence handed to nn.Linear) on every tagger call with this option')

    def _prep_input(self, xs, lengths):
        """pad_packed_sequence semantics: the output covers max(lengths) positions (NeuralArchitectures.py:115).
        ``xs`` may be a K-split pair (taggers._split_input): both parts are trimmed, the pair is returned."""
        x1, x2, B, Lin, _ = self._split_input(xs)
        maxlen = int(lengths.max()) if lengths is not None else Lin
        maxlen = min(maxlen, Lin)
        if x2 is not None:
            return (x1[:, :maxlen].contiguous(), x2[:, :maxlen].contiguous()), maxlen
        return x1[:, :maxlen].contiguous(), maxlen

    def _drop_seed(self):
        """A fresh 64-bit seed per dropout call, derived from torch's seed (torch.manual_seed makes runs repeatable)."""
        self._drop_calls += 1
        return (torch.initial_seed() * 1000003 + self._drop_calls * 7919) & 0x7FFFFFFFFFFFFFFF

    def _drop_in(self, xa, tag):
        """F.dropout on the RNN input (NeuralArchitectures.py:94); no mask kept: nothing upstream needs a gradient."""
        if not self.dropout_in:
            return xa
        out = self._ws.get('xdrop_' + tag, xa.shape[0], xa.shape[1], xa.dtype, xa.device)
        ops.dropout_fwd(xa, out, self.dropout_in, self._drop_seed())
        return out

    def _drop_out(self, h, tag):
        """F.dropout on the RNN output (NeuralArchitectures.py:119) -> (dropped copy, mask); `h` itself stays intact for the
        recurrence backward."""
        if not self.dropout_out:
            return h, None
        out = self._ws.get('hdrop_' + tag, h.shape[0], h.shape[1], h.dtype, h.device)
        mask = self._ws.get('hmask_' + tag, h.shape[0], h.shape[1], torch.uint8, h.device)
        ops.dropout_fwd(h, out, self.dropout_out, self._drop_seed(), mask=mask)
        return out, mask

    COSINE_WEIGHT = 0.1              # tot_loss = 0.1 * cos_loss + loss (models/CRF.py:335, :440)

    def _segment_tables(self, segments, xs, lengths, tags):
        """Host tables of the cosine auxiliary loss for this batch, validated before anything is launched (ops.segment_table), and the
        target-shape check of the reference's unmasked main loss (models/CRF.py:331-333): all three loss functions refuse targets that do
        not cover exactly max(lengths) positions."""
        x1, _, B, Lin, _ = self._split_input(xs)
        Lq = min(int(lengths.max()) if lengths is not None else Lin, Lin)
        tab = ops.segment_tables(segments, lengths, B, Lq, x1.device)
        if tags.shape[1] != Lq:
            n_in, n_tg = B * Lq, tags.numel()
            if self.loss_kind == L.LOSS_CE:
                raise ValueError(f'Expected input batch_size ({n_in}) to match target batch_size ({n_tg}).')
            if self.loss_kind == L.LOSS_FOCAL:
                raise ValueError(f'Target size (torch.Size([{n_tg}])) must be the same as input size (torch.Size([{n_in}]))')
            raise ValueError(f'Using a target size (torch.Size([{n_tg}])) that is different to the input size (torch.Size([{n_in}])) is '
                             'deprecated. Please ensure they have the same size.')
        if self.loss_kind == L.LOSS_BCE and tags.numel():
            # nn.BCELoss over ALL positions: the collater's pad -1 is refused upstream (fixture g21 err_bce_pad); pad 0 (the CRF collater's)
            # runs.  Targets still on the host (the collater's) are checked there; device targets cost one synchronisation per step
            lo, hi = tags.min(), tags.max()
            if float(lo) < 0.0 or float(hi) > 1.0:
                raise RuntimeError('all elements of target should be between 0 and 1')
        return tab

    def _cosine_fwd(self, tab, act, loss_out):
        """loss_out[0] += 0.1 * (mean cosine-embedding term over the batch's pairs) -> the kernels' workspace (None without a pair: the
        reference's cosine term is then the int 0)."""
        if tab.n_pair == 0:
            return None
        cos_out = self._ws.get('cos_out', 1, 2, torch.float32, act.device).view(-1)
        ws = ops.segment_cosine_fwd(act, tab, cos_out)
        loss_out[:1].add_(cos_out[:1], alpha=self.COSINE_WEIGHT)
        return ws

    def _cosine_bwd(self, tab, ws, dact):
        """the cosine term's gradient, added into the head's data gradient"""
        if ws is not None:
            ops.segment_cosine_bwd(tab, self.COSINE_WEIGHT * self.loss_grad_scale / tab.n_pair, dact, ws, accumulate=True)

    def _to_act(self, x):
        if isinstance(x, tuple):                                       # K-split pair: concat + cast in one pass over the two fp32 parts
            a, b = (t.reshape(-1, t.shape[-1]).to(torch.float32).contiguous() for t in x)
            D = a.shape[1] + b.shape[1]
            if D % 8 == 0:
                out = self._ws.get('xin_' + str(D), a.shape[0], D, self.compute_dtype, a.device)
                return ops.cast_concat(a, b, out)
            x = torch.cat((a, b), dim=1)                               # odd widths (timing features): the padded path below
        x2 = x.reshape(-1, x.shape[-1])
        if x2.dtype == torch.bfloat16 and self.compute_dtype == torch.bfloat16 and x2.shape[1] % 8 == 0:
            return x2.contiguous()                                     # already in the act dtype (prefetch.DevicePrefetcher wire_dtype='bf16'):
                                                                       # the same bits the cast below would produce from the fp32 batch
        if x2.shape[1] % 8:                                           # e.g. 768 + 2 timing features: zero columns up to a multiple of 8
            x2 = torch.nn.functional.pad(x2.to(torch.float32), (0, round_up(x2.shape[1], 8) - x2.shape[1]))
        if self.compute_dtype == torch.float32:
            return x2.to(torch.float32).contiguous()
        out = self._ws.get('xin_' + str(x2.shape[1]), x2.shape[0], x2.shape[1], torch.bfloat16, x.device)
        ops.cast(x2.to(torch.float32).contiguous(), out)
        return out


class BiLSTM(_RnnTaggerBase):
    """models/CRF.py:274-369."""
    takes_segments = True            # loss_and_grad(..., segments=): trainer.NativeTrainer(cosine_loss=True) passes batch['src_segments']

    def __init__(self, tagset_size, embedding_dim, hidden_dim, num_layers=1, bidirectional=True, dropout_in=0.0, dropout_out=0.0,
                 batch_first=True, LSTM=True, loss_fn='CrossEntropy', threshold=None, device=None, alpha=0.9, gamma=2,
                 compute_dtype=None, seed=None):
        super().__init__()
        self._init_common(loss_fn, threshold, alpha, gamma, compute_dtype)
        self._check_rnn_args(dropout_in, dropout_out, LSTM, bidirectional)
        self.embedding_dim, self.hidden_dim, self.tagset_size, self.num_layers = embedding_dim, hidden_dim, tagset_size, num_layers
        self.n_out = tagset_size if loss_fn == 'CrossEntropy' else 1
        gen = torch.Generator().manual_seed(torch.initial_seed() if seed is None else seed)
        groups, init, pads = _rnn_groups('model.', embedding_dim, hidden_dim, num_layers, gen)
        self._hp = round_up(hidden_dim, 8)
        cw, cb = _linear_init(self.n_out, 2 * hidden_dim, gen)
        groups.append([('classification.weight', (self.n_out, 2 * self._hp)), ('classification.bias', (self.n_out,))])
        init['classification.weight'], init['classification.bias'] = cw, cb
        if _head_pad(hidden_dim, 2):
            pads['classification.weight'] = _head_pad(hidden_dim, 2)
        self._init_flat(FlatLayout(groups, pads), init)
        self._rnn = _RnnStack(self, 'model.', embedding_dim, hidden_dim, num_layers, 'r')

    def _fwd(self, xs, lengths):
        x, Lq = self._prep_input(xs, lengths)
        first = x[0] if isinstance(x, tuple) else x
        B, dev = first.shape[0], first.device
        li32 = self._prep_lengths(lengths, B, Lq, dev)
        h, saved = self._rnn.forward(self._drop_in(self._to_act(x), 'r'), li32, B, Lq)
        h, hmask = self._drop_out(h, 'r')
        scores = self._ws.get('scores', B * Lq, self.n_out, torch.float32, dev)
        ops.head_fwd(h, self._w(self._flat, 'classification.weight'), self._w(self._flat, 'classification.bias'), scores)
        return dict(B=B, L=Lq, li32=li32, h=h, hmask=hmask, saved=saved, scores=scores.view(B, Lq, self.n_out))

    def loss_and_grad(self, xs, lengths, tags, want_grad=True, segments=None):
        """segments (one list of segment ends per document, the batch's 'src_segments'): the `segments=` branch of the reference (models/CRF.py:
        322-337) -- 0.1 x the cosine auxiliary loss over the encoder output is added, and the main loss runs over ALL B x max(len)
        positions, padded ones included (DESIGN.md "Cosine auxiliary segment loss")."""
        L.require_gpu()
        tab = self._segment_tables(segments, xs, lengths, tags) if segments is not None else None
        st = self._fwd(xs, lengths)
        dev, B, Lq = st['scores'].device, st['B'], st['L']
        tg = tags.to(device=dev, dtype=torch.float32).contiguous()
        if self.loss_kind == L.LOSS_CE and tg.shape[1] != Lq:
            # the reference reshapes x [B*maxlen, 2] against tags [B*L] (CRF.py:354) and fails on a size mismatch
            raise ValueError(f'Expected input batch_size ({B * Lq}) to match target batch_size ({tg.numel()}).')
        loss_out = torch.empty(2, dtype=torch.float32, device=dev)
        dsc = self._ws.get('dscores', B * Lq, self.n_out, torch.float32, dev) if want_grad else None
        # with segments the reference does not un-pad (CRF.py:331): every document counts max(len) rows (lengths = NULL)
        ops.tagger_loss(self.loss_kind, st['scores'], tg, st['li32'] if tab is None else None, self.alpha, self.gamma, loss_out, dsc)
        cos_ws = self._cosine_fwd(tab, st['h'], loss_out) if tab is not None else None
        if want_grad:
            ops.scale_(dsc, self.loss_grad_scale)
            g, lay = self.grad_flat(), self._layout
            ops.head_bwd_params(st['h'], dsc, lay.view(g, 'classification.weight'), lay.view(g, 'classification.bias'))
            self._grads_ready(*self._span_of('classification.weight', 'classification.bias'))
            dout = self._ws.get('dout', B * Lq, 2 * self._hp, self.compute_dtype, dev)
            ops.head_bwd_data(dsc, self._w(self._flat, 'classification.weight'), dout)
            self._cosine_bwd(tab, cos_ws, dout)
            if st['hmask'] is not None:
                ops.dropout_bwd(dout, dout, st['hmask'], self.dropout_out)
            self._rnn.backward(st['saved'], dout, st['li32'], B, Lq)
        return loss_out[0], st['scores']

    def loss(self, xs, lengths, tags, segments=None):
        """models/CRF.py:319-356."""
        if torch.is_grad_enabled() and any(p.requires_grad for p in self._flat_params.values()):
            return self._autograd_loss(lambda: self.loss_and_grad(xs, lengths, tags, True, segments)[0])
        return self.loss_and_grad(xs, lengths, tags, False, segments)[0].clone()

    def forward(self, xs, lenghts, threshold=0.4):
        """models/CRF.py:358-369."""
        L.require_gpu()
        with torch.no_grad():
            st = self._fwd(xs, lenghts)
            scores = st['scores'].clone()
            tags = self._decode(scores, st['li32'], lenghts, threshold)
        return scores, tags


class BiLSTMLateFusion(_RnnTaggerBase):
    """models/CRF.py:371-479: two independent RNNs, plain concat (there is no gate in the reference), one head.

    merge='gate' (extension, default 'concat'; DESIGN.md "Gated late-fusion merge"): the head reads m = z h1 + (1 - z) h2 with
    z = sigmoid([h1 ; h2] W_g^T + b_g), a learned per-unit choice between the two encoders, instead of [h1 ; h2].  Adds the parameters
    ``gate.weight`` [2H, 4H] and ``gate.bias`` [2H]; ``classification.weight`` is then [n_out, 2H].  Everything around the merge (loss,
    un-padding, decode, threshold, ``segments=``) is the concat mode's."""
    MERGES = ('concat', 'gate')
    takes_segments = True            # as BiLSTM
    concurrent_encoders = True       # model1 / model2 on two HIP streams (bitwise the same results).  Under a data-parallel hook too:
                                     # model2's spans are announced from inside `with stream(side)`, so the collective is issued
                                     # with the side stream current and waits on exactly the kernels that wrote the span (RCCL and
                                     # gloo both order a collective behind the stream that is current when it is issued); the host
                                     # order of the announcements -- model2's layers, then model1's -- is the same on every rank

    def _side_stream(self, dev):
        return ops.side_stream(dev, 0)

    def __init__(self, tagset_size, embedding_dim, hidden_dim, num_layers=1, bidirectional=True, dropout_in=0.0, dropout_out=0.0,
                 batch_first=True, LSTM=True, loss_fn='CrossEntropy', threshold=None, device=None, alpha=0.9, gamma=2,
                 compute_dtype=None, seed=None, merge='concat'):
        super().__init__()
        if merge not in self.MERGES:
            raise ValueError(f"merge must be one of {self.MERGES}, got {merge!r}")
        self.merge = merge
        self._init_common(loss_fn, threshold, alpha, gamma, compute_dtype)
        self._check_rnn_args(dropout_in, dropout_out, LSTM, bidirectional)
        self.embedding_dim, self.hidden_dim, self.tagset_size, self.num_layers = embedding_dim, hidden_dim, tagset_size, num_layers
        self.n_out = tagset_size if loss_fn == 'CrossEntropy' else 1
        gen = torch.Generator().manual_seed(torch.initial_seed() if seed is None else seed)
        g1, i1, p1 = _rnn_groups('model1.', embedding_dim[0], hidden_dim, num_layers, gen)
        g2, i2, p2 = _rnn_groups('model2.', embedding_dim[1], hidden_dim, num_layers, gen)
        H, Hp = hidden_dim, round_up(hidden_dim, 8)
        self._hp = Hp
        nblocks = 2 if merge == 'gate' else 4             # hidden vectors the head reads: the merged one | the concatenation
        cw, cb = _linear_init(self.n_out, nblocks * H, gen)
        groups = g1 + g2 + [[('classification.weight', (self.n_out, nblocks * Hp)), ('classification.bias', (self.n_out,))]]
        init = {**i1, **i2, 'classification.weight': cw, 'classification.bias': cb}
        pads = {**p1, **p2}
        if _head_pad(H, nblocks):
            pads['classification.weight'] = _head_pad(H, nblocks)
        if merge == 'gate':
            # drawn after the head's: a given seed leaves both encoders' initial weights as they are in concat mode.  Zero bias and a small
            # weight: z starts near 1/2, the merge near the mean of the two encoders
            init['gate.weight'], init['gate.bias'] = _linear_init(2 * H, 4 * H, gen)[0], torch.zeros(2 * H)
            groups.append([('gate.weight', (2 * Hp, 4 * Hp)), ('gate.bias', (2 * Hp,))])
            if Hp != H:                                    # padded units are inert: h = 0 there, so m, da and every pad gradient are exactly 0
                pads['gate.weight'] = [(0, 2, H, Hp), (1, 4, H, Hp)]
                pads['gate.bias'] = [(0, 2, H, Hp)]
        self._init_flat(FlatLayout(groups, pads), init)
        self._rnn1 = _RnnStack(self, 'model1.', embedding_dim[0], hidden_dim, num_layers, 'r1')
        self._rnn2 = _RnnStack(self, 'model2.', embedding_dim[1], hidden_dim, num_layers, 'r2')

    def _fwd(self, x1, x2, lengths):
        xa, Lq = self._prep_input(x1, lengths)
        xb, _ = self._prep_input(x2, lengths)
        B, H = xa.shape[0], self._hp
        li32 = self._prep_lengths(lengths, B, Lq, x1.device)
        # the two encoders are independent and each recurrence occupies a few dozen CUs: run the second one on a side stream
        side = self._side_stream(x1.device) if self.concurrent_encoders else None
        if side is not None:
            main = torch.cuda.current_stream(x1.device)
            self._weights()                            # a stale bf16 mirror is re-cast HERE, on the main stream, ahead of both encoders
            side.wait_stream(main)
            with torch.cuda.stream(side):
                h2, s2 = self._rnn2.forward(self._drop_in(self._to_act(xb), 'r2'), li32, B, Lq)
            h1, s1 = self._rnn1.forward(self._drop_in(self._to_act(xa), 'r1'), li32, B, Lq)
            main.wait_stream(side)
        else:
            h1, s1 = self._rnn1.forward(self._drop_in(self._to_act(xa), 'r1'), li32, B, Lq)
            h2, s2 = self._rnn2.forward(self._drop_in(self._to_act(xb), 'r2'), li32, B, Lq)
        h1, m1 = self._drop_out(h1, 'r1')
        h2, m2 = self._drop_out(h2, 'r2')
        if self.merge == 'gate':
            return self._fwd_gate(B, Lq, li32, h1, h2, s1, s2, m1, m2)
        cat = self._ws.get('cat', B * Lq, 4 * H, self.compute_dtype, x1.device)
        cat[:, :2 * H].copy_(h1)                       # torch.cat((x1, x2), axis=2), models/CRF.py:425
        cat[:, 2 * H:].copy_(h2)
        scores = self._ws.get('scores', B * Lq, self.n_out, torch.float32, x1.device)
        ops.head_fwd(cat, self._w(self._flat, 'classification.weight'), self._w(self._flat, 'classification.bias'), scores)
        return dict(B=B, L=Lq, li32=li32, cat=cat, s1=s1, s2=s2, m1=m1, m2=m2, scores=scores.view(B, Lq, self.n_out))

    def _fwd_gate(self, B, Lq, li32, h1, h2, s1, s2, m1, m2):
        """The gated merge and the head on it (both encoders joined on the issuing stream).  a = h1 W_g[:, :2H]^T + h2 W_g[:, 2H:]^T + b_g as
        two GEMMs on the column halves of W_g: no concatenated buffer exists in this mode.  The second product reaches the first call as
        its residual operand, from a buffer of its own (the bias + residual epilogue of every NT kernel is what the suite tests)."""
        N, W, dt, dev = B * Lq, 2 * self._hp, self.compute_dtype, h1.device
        wg = self._w(self._weights(), 'gate.weight')
        a2 = self._ws.get('gate_a2', N, W, dt, dev)
        ops.linear_fwd(h2, wg[:, W:], None, a2)
        a = self._ws.get('gate_a', N, W, dt, dev)
        ops.linear_fwd(h1, wg[:, :W], self._w(self._flat, 'gate.bias'), a, residual=a2)
        m = self._ws.get('gate_m', N, W, dt, dev)
        ops.gate_merge_fwd(a, h1, h2, m)
        scores = self._ws.get('scores', N, self.n_out, torch.float32, dev)
        ops.head_fwd(m, self._w(self._flat, 'classification.weight'), self._w(self._flat, 'classification.bias'), scores)
        return dict(B=B, L=Lq, li32=li32, cat=m, a=a, h1=h1, h2=h2, s1=s1, s2=s2, m1=m1, m2=m2, scores=scores.view(B, Lq, self.n_out))

    def _bwd_gate(self, st, dm, d1, d2):
        """dm -> d1, d2 (the two encoders' output gradients) and the gate's parameter gradients, announced before the encoders start."""
        N, W, dt, dev = dm.shape[0], 2 * self._hp, self.compute_dtype, dm.device
        g, lay = self.grad_flat(), self._layout
        da = self._ws.get('gate_da', N, W, dt, dev)
        p1 = self._ws.get('gate_p1', N, W, dt, dev)
        p2 = self._ws.get('gate_p2', N, W, dt, dev)
        ops.gate_merge_bwd(st['a'], st['h1'], st['h2'], dm, da, p1, p2)
        dwg = lay.view(g, 'gate.weight')
        ops.colsum(da, lay.view(g, 'gate.bias'))
        ops.linear_wgrad(da, st['h1'], dwg[:, :W])
        ops.linear_wgrad(da, st['h2'], dwg[:, W:])
        self._grads_ready(*self._span_of('gate.weight', 'gate.bias'))
        # d1 = dm z + da W_g[:, :2H]: the kernel's part comes in as the residual operand (act-dtype NN output + residual: tested for every kernel)
        wg = self._w(self._weights(), 'gate.weight')
        ops.linear_dgrad(da, wg[:, :W], d1, residual=p1)
        ops.linear_dgrad(da, wg[:, W:], d2, residual=p2)

    def loss_and_grad(self, x1, x2, lengths, tags, want_grad=True, segments=None):
        """segments: as BiLSTM.loss_and_grad (models/CRF.py:427-442); the cosine loss reads the concatenation of the two encoders' outputs
        (merge='gate': the merged output)."""
        L.require_gpu()
        tab = self._segment_tables(segments, x1, lengths, tags) if segments is not None else None
        st = self._fwd(x1, x2, lengths)
        dev, B, Lq, H = x1.device, st['B'], st['L'], self._hp
        tg = tags.to(device=dev, dtype=torch.float32).contiguous()
        loss_out = torch.empty(2, dtype=torch.float32, device=dev)
        dsc = self._ws.get('dscores', B * Lq, self.n_out, torch.float32, dev) if want_grad else None
        ops.tagger_loss(self.loss_kind, st['scores'], tg, st['li32'] if tab is None else None, self.alpha, self.gamma, loss_out, dsc)
        cos_ws = self._cosine_fwd(tab, st['cat'], loss_out) if tab is not None else None
        if want_grad:
            ops.scale_(dsc, self.loss_grad_scale)
            g, lay = self.grad_flat(), self._layout
            ops.head_bwd_params(st['cat'], dsc, lay.view(g, 'classification.weight'), lay.view(g, 'classification.bias'))
            self._grads_ready(*self._span_of('classification.weight', 'classification.bias'))
            d1 = self._ws.get('dout1', B * Lq, 2 * H, self.compute_dtype, dev)
            d2 = self._ws.get('dout2', B * Lq, 2 * H, self.compute_dtype, dev)
            if self.merge == 'gate':
                dm = self._ws.get('gate_dm', B * Lq, 2 * H, self.compute_dtype, dev)
                ops.head_bwd_data(dsc, self._w(self._flat, 'classification.weight'), dm)
                self._cosine_bwd(tab, cos_ws, dm)
                self._bwd_gate(st, dm, d1, d2)
            else:
                dcat = self._ws.get('dcat', B * Lq, 4 * H, self.compute_dtype, dev)
                ops.head_bwd_data(dsc, self._w(self._flat, 'classification.weight'), dcat)
                self._cosine_bwd(tab, cos_ws, dcat)
                d1.copy_(dcat[:, :2 * H])
                d2.copy_(dcat[:, 2 * H:])
            if st['m1'] is not None:
                ops.dropout_bwd(d1, d1, st['m1'], self.dropout_out)
                ops.dropout_bwd(d2, d2, st['m2'], self.dropout_out)
            side = self._side_stream(dev) if self.concurrent_encoders else None
            if side is not None:
                main = torch.cuda.current_stream(dev)
                self._weights()                        # see _fwd: never let the side stream be the one that refreshes the mirror
                side.wait_stream(main)
                with torch.cuda.stream(side):
                    self._rnn2.backward(st['s2'], d2, st['li32'], B, Lq)
                self._rnn1.backward(st['s1'], d1, st['li32'], B, Lq)
                main.wait_stream(side)
            else:
                self._rnn1.backward(st['s1'], d1, st['li32'], B, Lq)
                self._rnn2.backward(st['s2'], d2, st['li32'], B, Lq)
        return loss_out[0], st['scores']

    def loss(self, x1, x2, lengths, tags, segments=None):
        """models/CRF.py:420-461."""
        if torch.is_grad_enabled() and any(p.requires_grad for p in self._flat_params.values()):
            return self._autograd_loss(lambda: self.loss_and_grad(x1, x2, lengths, tags, True, segments)[0])
        return self.loss_and_grad(x1, x2, lengths, tags, False, segments)[0].clone()

    def forward(self, x1, x2, lenghts, threshold=0.4):
        """models/CRF.py:463-479."""
        L.require_gpu()
        with torch.no_grad():
            st = self._fwd(x1, x2, lenghts)
            scores = st['scores'].clone()
            tags = self._decode(scores, st['li32'], lenghts, threshold)
        return scores, tags


class BiRnnCrf(_RnnTaggerBase):
    """models/CRF.py:243-272 composed with CRF (:98-240): RNN -> fc(2H -> tags+2) -> CRF NLL / Viterbi.

    decode='marginal' (extension, default 'viterbi'; DESIGN.md "CRF posterior-marginal decode"): ``forward`` scores every sentence with the
    logit of its posterior marginal P(y_t = 1 | x) (mts_crf_marginals) and decodes by ``sigmoid(score) > th`` like the other taggers, so the
    threshold sweeps apply.  It needs tagset_size == 2 (class 1 must be a real tag).  ``decode`` is not state: the parameters, the loss and
    the state_dict are those of the default model."""
    crf_head = True
    crf_architecture = 'biLSTMCRF'
    DECODES = ('viterbi', 'marginal')
    _GUARDED_ENTRY_POINTS = _TaggerBase._GUARDED_ENTRY_POINTS + ('marginal_scores',)

    def __init__(self, tagset_size, embedding_dim, hidden_dim, num_layers=1, bidirectional=True, dropout_in=0.0, dropout_out=0.0,
                 batch_first=True, LSTM=True, architecture='rnn', compute_dtype=None, seed=None, decode='viterbi'):
        super().__init__()
        if decode not in self.DECODES:
            raise ValueError(f'decode must be one of {self.DECODES}, got {decode!r}')
        if decode == 'marginal' and tagset_size != 2:
            raise ValueError(f"decode='marginal' needs tagset_size == 2 (class 1 must be a real tag), got {tagset_size}")
        self.decode = decode
        self._init_common('CrossEntropy', None, 0.9, 2, compute_dtype)
        self._check_rnn_args(dropout_in, dropout_out, LSTM, bidirectional)
        self.embedding_dim, self.hidden_dim, self.tagset_size, self.num_layers = embedding_dim, hidden_dim, tagset_size, num_layers
        self.num_tags = tagset_size + 2                       # models/CRF.py:108-110
        self.start_idx, self.stop_idx = self.num_tags - 2, self.num_tags - 1
        if self.num_tags > 4:
            raise NotImplementedError('CRF head supports tagset_size <= 2 (fused head kernels cover <= 4 outputs)')
        gen = torch.Generator().manual_seed(torch.initial_seed() if seed is None else seed)
        groups, init, pads = _rnn_groups('model.', embedding_dim, hidden_dim, num_layers, gen)
        self._hp = round_up(hidden_dim, 8)
        C = self.num_tags
        fw, fb = _linear_init(C, 2 * hidden_dim, gen)
        trans = torch.randn(C, C, generator=gen)
        trans[self.start_idx, :] = IMPOSSIBLE                 # models/CRF.py:115-117
        trans[:, self.stop_idx] = IMPOSSIBLE
        groups.append([('crf.fc.weight', (C, 2 * self._hp)), ('crf.fc.bias', (C,))])
        groups.append([('crf.transitions', (C, C))])
        init.update({'crf.fc.weight': fw, 'crf.fc.bias': fb, 'crf.transitions': trans})
        if _head_pad(hidden_dim, 2):
            pads['crf.fc.weight'] = _head_pad(hidden_dim, 2)
        self._init_flat(FlatLayout(groups, pads), init)
        self._rnn = _RnnStack(self, 'model.', embedding_dim, hidden_dim, num_layers, 'r')

    def _fwd(self, xs, lengths):
        x, Lq = self._prep_input(xs, lengths)
        first = x[0] if isinstance(x, tuple) else x
        B, dev = first.shape[0], first.device
        li32 = self._prep_lengths(lengths, B, Lq, dev)
        h, saved = self._rnn.forward(self._drop_in(self._to_act(x), 'r'), li32, B, Lq)
        h, hmask = self._drop_out(h, 'r')
        feats = self._ws.get('feats', B * Lq, self.num_tags, torch.float32, dev)
        ops.head_fwd(h, self._w(self._flat, 'crf.fc.weight'), self._w(self._flat, 'crf.fc.bias'), feats)
        return dict(B=B, L=Lq, li32=li32, h=h, hmask=hmask, saved=saved, feats=feats.view(B, Lq, self.num_tags))

    def loss_and_grad(self, xs, lengths, tags, want_grad=True):
        L.require_gpu()
        st = self._fwd(xs, lengths)
        dev, B, Lq, C = st['feats'].device, st['B'], st['L'], self.num_tags
        tg = tags.to(device=dev, dtype=torch.float32).contiguous()
        loss_out = torch.empty(2, dtype=torch.float32, device=dev)
        g, lay = self.grad_flat(), self._layout
        dfe = self._ws.get('dfeats', B * Lq, C, torch.float32, dev) if want_grad else None
        ops.crf_nll(st['feats'], tg, st['li32'], self._w(self._flat, 'crf.transitions'), loss_out,
                    dfe.view(B, Lq, C) if want_grad else None, lay.view(g, 'crf.transitions') if want_grad else None)
        if want_grad:
            ops.scale_(dfe, self.loss_grad_scale)
            ops.scale_(lay.view(g, 'crf.transitions'), self.loss_grad_scale)
            ops.head_bwd_params(st['h'], dfe, lay.view(g, 'crf.fc.weight'), lay.view(g, 'crf.fc.bias'))
            self._grads_ready(*self._span_of('crf.fc.weight', 'crf.transitions'))
            dout = self._ws.get('dout', B * Lq, 2 * self._hp, self.compute_dtype, dev)
            ops.head_bwd_data(dfe, self._w(self._flat, 'crf.fc.weight'), dout)
            if st['hmask'] is not None:
                ops.dropout_bwd(dout, dout, st['hmask'], self.dropout_out)
            self._rnn.backward(st['saved'], dout, st['li32'], B, Lq)
        return loss_out[0], st['feats']

    def loss(self, xs, lengths, tags):
        """models/CRF.py:261-265."""
        if torch.is_grad_enabled() and any(p.requires_grad for p in self._flat_params.values()):
            return self._autograd_loss(lambda: self.loss_and_grad(xs, lengths, tags, True)[0])
        return self.loss_and_grad(xs, lengths, tags, False)[0].clone()

    def _marginal_scores(self, st):
        B, Lq = st['B'], st['L']
        scores = torch.empty(B, Lq, 1, dtype=torch.float32, device=st['feats'].device)
        ops.crf_marginals(st['feats'], st['li32'], self._w(self._flat, 'crf.transitions'), scores.view(B, Lq), cls=1)
        return scores

    def marginal_scores(self, xs, lengths):
        """-> [B, Lq, 1] fp32: the logit of P(y_t = 1 | x) clamped to +-80, 0 past a document's length (either decode mode)."""
        L.require_gpu()
        with torch.no_grad():
            return self._marginal_scores(self._fwd(xs, lengths))

    def forward(self, xs, lenghts, threshold=0.4):
        """models/CRF.py:267-272 -> (best_score [B], best_paths list of int lists).  decode='marginal': (scores [B, Lq, 1], list of
        per-document bool lists) by sigmoid(score) > th, ``.th`` over the argument, as BiLSTM.forward."""
        L.require_gpu()
        if self.decode == 'marginal':
            with torch.no_grad():
                st = self._fwd(xs, lenghts)
                scores = self._marginal_scores(st)
                tags = self._decode(scores, st['li32'], lenghts, threshold)
            return scores, tags
        with torch.no_grad():
            st = self._fwd(xs, lenghts)
            B, Lq = st['B'], st['L']
            score = torch.empty(B, dtype=torch.float32, device=st['feats'].device)
            paths = torch.empty(B, Lq, dtype=torch.int32, device=st['feats'].device)
            ops.crf_viterbi(st['feats'], st['li32'], self._w(self._flat, 'crf.transitions'), score, paths)
            ph = paths.cpu().numpy()
            L.check_async()            # synchronised by the copy: report a CU-pair LSTM timeout of this forward instead of its paths
            lens = [int(v) for v in (lenghts.tolist() if lenghts is not None else [Lq] * B)]
        return score, [ph[i, :min(lens[i], Lq)].tolist() for i in range(B)]


_PAIR_LENGTHS_CACHE = {}


class SheikhBiLSTM(_RnnTaggerBase):
    """models/CRF.py:980-1041: Sheikh et al.'s change-detection BiLSTM.  The boundary after sentence t is scored from the forward state at
    t and the backward state at t + 1:  s[b, t] = forward_dense(h[b, t, :H]) . backward_dense(h[b, t + 1, H:]),  t < max(len) - 1, and
    ``forward`` appends one step of ones.  Loss: BCELoss(1 - sigmoid(s), 1 - y) over t < len_b - 1 (= BCE on (s, y); whatever ``loss_fn``
    says, :1002 overwrites it).  ``.th`` is never set by the constructor (TextSegmenter.test_step assigns it): ``forward`` before that
    raises the reference's AttributeError.  The reference's ``classification`` Linear(2H, 1) is read by no method: this module does not own
    it and drops it on load."""
    grad_hooks_cover_all = False     # gradients are not announced span by span: NativeTrainer all-reduces after the backward
    DEAD_KEYS = ('classification.weight', 'classification.bias')

    def __init__(self, tagset_size, embedding_dim, hidden_dim, num_layers, dropout_in=0.5, dropout_attention=0.0, batch_first=True,
                 loss_fn='BinaryCrossEntropy', alpha=0.9, gamma=2, compute_dtype=None, seed=None):
        super().__init__()
        if loss_fn not in ('BinaryCrossEntropy', 'FocalLoss'):
            raise ValueError('Choose one of FocalLoss or BinaryCrossEntropy as loss function')    # models/CRF.py:999
        self._init_common('BinaryCrossEntropy', None, alpha, gamma, compute_dtype)                # :1002: nn.BCELoss in both cases
        del self.th                                                                               # the reference's constructor never sets it
        self._check_rnn_args(dropout_in, dropout_attention, True, True)                           # RNN(..., dropout_in, dropout_attention, LSTM=True)
        self.embedding_dim, self.hidden_dim, self.tagset_size, self.num_layers = embedding_dim, hidden_dim, tagset_size, num_layers
        self.n_out = 1
        gen = torch.Generator().manual_seed(torch.initial_seed() if seed is None else seed)
        groups, init, pads = _rnn_groups('lstm.', embedding_dim, hidden_dim, num_layers, gen)
        H, Hp = hidden_dim, round_up(hidden_dim, 8)
        self._hp = Hp
        fw, fb = _linear_init(H, H, gen)
        bw, bb = _linear_init(H, H, gen)
        groups.append([('forward_dense.weight', (Hp, Hp))])
        groups.append([('backward_dense.weight', (Hp, Hp))])
        groups.append([('forward_dense.bias', (Hp,)), ('backward_dense.bias', (Hp,))])   # adjacent: one column sum over dF | dG gives both
        init.update({'forward_dense.weight': fw, 'forward_dense.bias': fb, 'backward_dense.weight': bw, 'backward_dense.bias': bb})
        if Hp != H:                                    # padded units are inert: zero rows / columns / biases -> F, G and their gradients are 0 there
            for n in ('forward_dense', 'backward_dense'):
                pads[n + '.weight'] = [(0, 1, H, Hp), (1, 1, H, Hp)]
                pads[n + '.bias'] = [(0, 1, H, Hp)]
        self._init_flat(FlatLayout(groups, pads), init)
        self._rnn = _RnnStack(self, 'lstm.', embedding_dim, hidden_dim, num_layers, 'r')
        self._register_load_state_dict_pre_hook(self._drop_dead_keys)

    @staticmethod
    def _drop_dead_keys(state_dict, prefix, *args):
        """A reference checkpoint carries classification.{weight,bias} (Linear(2H, 1), :994 / :997), which no method reads: ignore them."""
        for k in SheikhBiLSTM.DEAD_KEYS:
            state_dict.pop(prefix + k, None)

    @staticmethod
    def _pair_lengths(lengths, li32):
        """max(len - 1, 0) per document on the device: the rows the loss averages.  Cached next to taggers._prep_lengths' entry (one small
        upload per distinct host length vector, none per step)."""
        if lengths is None or not (lengths.device.type == 'cpu' and lengths.numel() <= 4096):
            return (li32 - 1).clamp_(min=0)
        key = (tuple(lengths.tolist()), str(li32.device))
        hit = _PAIR_LENGTHS_CACHE.get(key)
        if hit is None:
            if len(_PAIR_LENGTHS_CACHE) > 64:
                _PAIR_LENGTHS_CACHE.clear()
            hit = _PAIR_LENGTHS_CACHE[key] = (lengths.to(torch.int32) - 1).clamp_(min=0).to(li32.device).contiguous()
        return hit

    def _fwd(self, xs, lengths):
        x, Lq = self._prep_input(xs, lengths)
        first = x[0] if isinstance(x, tuple) else x
        B, dev, Hp = first.shape[0], first.device, self._hp
        li32 = self._prep_lengths(lengths, B, Lq, dev)
        h, saved = self._rnn.forward(self._drop_in(self._to_act(x), 'r'), li32, B, Lq)
        h, hmask = self._drop_out(h, 'r')
        wf, pf = self._weights(), self._flat
        # F = forward_dense(forward states) | G = backward_dense(backward states): the two halves of one [N, 2Hp] buffer, every row (the
        # reference's x[:, :-1] / x[:, 1:] slices are the pairing of the score kernel)
        FG = self._ws.get('FG', B * Lq, 2 * Hp, self.compute_dtype, dev)
        ops.linear_fwd(h[:, :Hp], self._w(wf, 'forward_dense.weight'), self._w(pf, 'forward_dense.bias'), FG[:, :Hp])
        ops.linear_fwd(h[:, Hp:], self._w(wf, 'backward_dense.weight'), self._w(pf, 'backward_dense.bias'), FG[:, Hp:])
        scores = self._ws.get('scores', B * Lq, 1, torch.float32, dev)
        ops.pair_score_fwd(FG[:, :Hp], FG[:, Hp:], B, Lq, scores)
        return dict(B=B, L=Lq, li32=li32, h=h, hmask=hmask, saved=saved, FG=FG, scores=scores.view(B, Lq, 1))

    def loss_and_grad(self, xs, lengths, tags, want_grad=True):
        L.require_gpu()
        st = self._fwd(xs, lengths)
        dev, B, Lq, Hp = st['scores'].device, st['B'], st['L'], self._hp
        tg = tags.to(device=dev, dtype=torch.float32).contiguous()
        loss_out = torch.empty(2, dtype=torch.float32, device=dev)
        dsc = self._ws.get('dscores', B * Lq, 1, torch.float32, dev) if want_grad else None
        # the un-pad loop of :1016-1019 keeps t < len_b - 1; mts_tagger_loss writes 0 into dscores for every row it does not average
        ops.tagger_loss(L.LOSS_BCE, st['scores'], tg, self._pair_lengths(lengths, st['li32']), self.alpha, self.gamma, loss_out, dsc)
        if Lq <= 1:
            loss_out[:1].fill_(float('nan'))           # every document of length <= 1: BCELoss over an empty tensor is NaN upstream (the
                                                       # kernel's mean over zero rows is 0); dscores is all zero, and so is every gradient
        if want_grad:
            ops.scale_(dsc, self.loss_grad_scale)
            g, lay, wf = self.grad_flat(), self._layout, self._weights()
            FG, h = st['FG'], st['h']
            dFG = self._ws.get('dFG', B * Lq, 2 * Hp, self.compute_dtype, dev)
            ops.pair_score_bwd(FG[:, :Hp], FG[:, Hp:], dsc, B, Lq, dFG[:, :Hp], dFG[:, Hp:])
            off, n = lay.span('forward_dense.bias', 'backward_dense.bias')
            ops.colsum(dFG, g[off:off + n])
            ops.linear_wgrad(dFG[:, :Hp], h[:, :Hp], lay.view(g, 'forward_dense.weight'))
            ops.linear_wgrad(dFG[:, Hp:], h[:, Hp:], lay.view(g, 'backward_dense.weight'))
            dout = self._ws.get('dout', B * Lq, 2 * Hp, self.compute_dtype, dev)
            ops.linear_dgrad(dFG[:, :Hp], self._w(wf, 'forward_dense.weight'), dout[:, :Hp])
            ops.linear_dgrad(dFG[:, Hp:], self._w(wf, 'backward_dense.weight'), dout[:, Hp:])
            if st['hmask'] is not None:
                ops.dropout_bwd(dout, dout, st['hmask'], self.dropout_out)
            self._rnn.backward(st['saved'], dout, st['li32'], B, Lq)
        return loss_out[0], st['scores']

    def loss(self, inputs, lengths, tags):
        """models/CRF.py:1005-1023 (no ``segments`` argument: TextSegmenter.training_step falls back on the TypeError, as upstream)."""
        if torch.is_grad_enabled() and any(p.requires_grad for p in self._flat_params.values()):
            return self._autograd_loss(lambda: self.loss_and_grad(inputs, lengths, tags, True)[0])
        return self.loss_and_grad(inputs, lengths, tags, False)[0].clone()

    def forward(self, inputs, lenghts, threshold=0.4):
        """models/CRF.py:1025-1041: scores [B, max(len), 1] with the appended step of ones, and the lists of 1 - sigmoid(s) < th."""
        if self.th is not None:                        # AttributeError until .th is assigned, as upstream (:1036)
            threshold = self.th
        L.require_gpu()
        with torch.no_grad():
            st = self._fwd(inputs, lenghts)
            scores = st['scores'].clone()
            B, Lq, _ = scores.shape
            tags = torch.empty(B, Lq, dtype=torch.uint8, device=scores.device)
            ops.greedy_decode(scores, st['li32'], 1.0 - threshold, tags)     # sigmoid(s) > 1 - th  <=>  1 - sigmoid(s) < th, strict
            tags_h = tags.cpu().numpy().astype(bool)
            L.check_async()
            lens = [int(v) for v in (lenghts.tolist() if lenghts is not None else [Lq] * B)]
        return scores, [tags_h[i, :lens[i]].tolist() for i in range(B)]


class SwitchBiLSTM(_RnnTaggerBase):
    """models/CRF.py:1046-1270: the domain-adaptation BiLSTM.  ``domains`` (one 0 / 1 / bool per document, the collater's
    ``batch['domain']``) picks, per document, one of two heads (``switch_dense_adapt``: 'dense') or, per batch, one of two encoders
    (``switch_lstm_adapt``: 'lstm'); with neither flag this is ``BiLSTM`` (state_dict keys ``model.`` / ``classification.``) and ``domains``
    is ignored, though still iterated.  State_dict keys per mode as upstream: dense ``model.`` + ``classification_1.`` + ``classification_2.``;
    lstm ``model_1.`` + ``model_2.`` + ``classification.``.

    dense, reproduced as it is (DESIGN.md "Domain-switched heads"): with idx1 = the documents whose domain is truthy and idx2 = the rest,
    a mixed batch runs BOTH heads over the whole batch and ``regroup`` assigns out[idx1[k]] = head_1(h)[k], out[idx2[k]] = head_2(h)[k]:
    document i is scored from the encoder rows of document rank(i), its position inside its own group, not from its own rows.  Document r is
    therefore read by up to two documents (idx1[r] and idx2[r]); documents r >= max(len(idx1), len(idx2)) are read by none and get a zero
    data gradient; rows at or past the SOURCE document's length are 0, so the score there is the bias.  The loss un-pads row i by lengths[i]
    against tags[i] as BiLSTM does.  A single-domain batch goes through classification_1 (all truthy) or classification_2 with its own rows.

    lstm: a single-domain batch runs model_1 (all truthy) or model_2; a mixed batch raises the AttributeError the reference dies with
    (:1146 hands RNN a list of lengths).

    The parameters a batch does not read (the other head / encoder) keep ``grad is None`` through ``loss().backward()``, as upstream, so a
    torch optimizer skips them; in ``grad_flat()`` their spans are zeros (``_unused_params`` names them for the autograd bridge).
    ``domain_learning=True`` computes a domain loss upstream and discards it (:1159-1162), and no TextSegmenter option reaches it: refused."""

    UPSTREAM_MIXED_LSTM = "'list' object has no attribute 'data'"      # fixture g20 lstm_mixed_msg
    takes_domains = True             # loss_and_grad(xs, lengths, tags, domains): trainer.NativeTrainer passes batch['domain']

    def __init__(self, tagset_size, embedding_dim, hidden_dim, num_layers=1, bidirectional=True, dropout_in=0.0, dropout_out=0.0,
                 batch_first=True, LSTM=True, loss_fn='CrossEntropy', threshold=None, device=None, alpha=0.9, gamma=2, bias_adapt=False,
                 switch_lstm_adapt=False, switch_dense_adapt=False, domain_learning=False, compute_dtype=None, seed=None):
        super().__init__()
        self._init_common(loss_fn, threshold, alpha, gamma, compute_dtype)
        self._check_rnn_args(dropout_in, dropout_out, LSTM, bidirectional)
        if domain_learning:
            raise NotImplementedError('domain_learning=True (models/CRF.py:1119-1122, :1159-1162): the reference computes a domain loss and '
                                      'discards it, and no TextSegmenter option reaches it; there is no behaviour to reproduce')
        self.embedding_dim, self.hidden_dim, self.tagset_size, self.num_layers = embedding_dim, hidden_dim, tagset_size, num_layers
        self.n_out = tagset_size if loss_fn == 'CrossEntropy' else 1
        self.switch = 'lstm' if switch_lstm_adapt else ('dense' if switch_dense_adapt else 0)      # :1061-1110
        self.dl = False
        gen = torch.Generator().manual_seed(torch.initial_seed() if seed is None else seed)
        self._hp = Hp = round_up(hidden_dim, 8)
        groups, init, pads = [], {}, {}
        prefixes = ('model_1.', 'model_2.') if self.switch == 'lstm' else ('model.',)
        for pre in prefixes:
            g, i, p = _rnn_groups(pre, embedding_dim, hidden_dim, num_layers, gen)
            groups += g
            init.update(i)
            pads.update(p)
        heads = ('classification_1', 'classification_2') if self.switch == 'dense' else ('classification',)
        for h in heads:
            init[h + '.weight'], init[h + '.bias'] = _linear_init(self.n_out, 2 * hidden_dim, gen)
            if _head_pad(hidden_dim, 2):
                pads[h + '.weight'] = _head_pad(hidden_dim, 2)
        # one group: the two heads' weights back to back = the kernels' stacked w [2, n_out, 2Hp], then the biases = bias [2, n_out]
        groups.append([(h + '.weight', (self.n_out, 2 * Hp)) for h in heads] + [(h + '.bias', (self.n_out,)) for h in heads])
        self._heads = heads
        self._init_flat(FlatLayout(groups, pads), init)
        self._stacks = {pre: _RnnStack(self, pre, embedding_dim, hidden_dim, num_layers, tag)
                        for pre, tag in zip(prefixes, ('r1', 'r2') if self.switch == 'lstm' else ('r',))}
        self._unused_params = frozenset()

    def _stack_names(self, pre):
        return f'{pre}rnn.weight_ih_l0', f'{pre}rnn.bias_hh_l{self.num_layers - 1}_reverse'

    def _route(self, domains):
        """-> (encoder prefix, names of the parameters this batch does not read).  Iterates ``domains`` as separate_domains does (:1124-1130):
        None raises TypeError."""
        truthy = [bool(d) for d in domains]
        any1, any2 = any(truthy), not all(truthy)
        if self.switch == 'lstm':
            if any1 and any2:
                raise AttributeError(self.UPSTREAM_MIXED_LSTM)
            pre = 'model_1.' if any1 else 'model_2.'
            other = 'model_2.' if any1 else 'model_1.'
            return pre, frozenset(n for n in self._layout.entries if n.startswith(other))
        if self.switch == 'dense' and not (any1 and any2):
            other = 'classification_2' if any1 else 'classification_1'
            return 'model.', frozenset((other + '.weight', other + '.bias'))
        return 'model.', frozenset()

    def _head_w(self, flat):
        return self._wspan(flat, self._heads[0] + '.weight', self._heads[-1] + '.weight', 2 * self.n_out, 2 * self._hp).view(2, self.n_out, 2 * self._hp)

    def _head_b(self, flat):
        return self._wspan(flat, self._heads[0] + '.bias', self._heads[-1] + '.bias', 2, self.n_out)

    def _fwd(self, xs, lengths, domains):
        pre, unused = self._route(domains)
        x, Lq = self._prep_input(xs, lengths)
        first = x[0] if isinstance(x, tuple) else x
        B, dev = first.shape[0], first.device
        li32 = self._prep_lengths(lengths, B, Lq, dev)
        rnn = self._stacks[pre]
        h, saved = rnn.forward(self._drop_in(self._to_act(x), rnn.tag), li32, B, Lq)
        h, hmask = self._drop_out(h, rnn.tag)
        scores = self._ws.get('scores', B * Lq, self.n_out, torch.float32, dev)
        if self.switch == 'dense':
            ops.switch_head_fwd(h, self._head_w(self._flat), self._head_b(self._flat), domains, B, Lq, scores)
        else:
            ops.head_fwd(h, self._w(self._flat, 'classification.weight'), self._w(self._flat, 'classification.bias'), scores)
        return dict(B=B, L=Lq, li32=li32, h=h, hmask=hmask, saved=saved, rnn=rnn, unused=unused, scores=scores.view(B, Lq, self.n_out))

    def loss_and_grad(self, xs, lengths, tags, domains, want_grad=True):
        L.require_gpu()
        st = self._fwd(xs, lengths, domains)
        dev, B, Lq = st['scores'].device, st['B'], st['L']
        tg = tags.to(device=dev, dtype=torch.float32).contiguous()
        if self.loss_kind == L.LOSS_CE and tg.shape[1] != Lq:
            raise ValueError(f'Expected input batch_size ({B * Lq}) to match target batch_size ({tg.numel()}).')     # as BiLSTM (:1224)
        loss_out = torch.empty(2, dtype=torch.float32, device=dev)
        dsc = self._ws.get('dscores', B * Lq, self.n_out, torch.float32, dev) if want_grad else None
        ops.tagger_loss(self.loss_kind, st['scores'], tg, st['li32'], self.alpha, self.gamma, loss_out, dsc)
        if want_grad:
            self._unused_params = st['unused']
            ops.scale_(dsc, self.loss_grad_scale)
            g, lay = self.grad_flat(), self._layout
            dout = self._ws.get('dout', B * Lq, 2 * self._hp, self.compute_dtype, dev)
            if self.switch == 'dense':
                # the head no document uses is written as exact zeros by the kernel: its span is announced like every other
                ops.switch_head_bwd_params(st['h'], dsc, domains, B, Lq, self._head_w(g), self._head_b(g))
                self._grads_ready(*self._span_of(self._heads[0] + '.weight', self._heads[-1] + '.bias'))
                ops.switch_head_bwd_data(dsc, self._head_w(self._flat), domains, B, Lq, dout)
            else:
                ops.head_bwd_params(st['h'], dsc, lay.view(g, 'classification.weight'), lay.view(g, 'classification.bias'))
                self._grads_ready(*self._span_of('classification.weight', 'classification.bias'))
                ops.head_bwd_data(dsc, self._w(self._flat, 'classification.weight'), dout)
            if self.switch == 'lstm':                      # the encoder this batch did not run: zero gradient, announced
                other = next(p for p in self._stacks if p != st['rnn'].prefix)
                a, b = self._span_of(*self._stack_names(other))
                g[a:b].zero_()
                self._grads_ready(a, b)
            if st['hmask'] is not None:
                ops.dropout_bwd(dout, dout, st['hmask'], self.dropout_out)
            st['rnn'].backward(st['saved'], dout, st['li32'], B, Lq)
        return loss_out[0], st['scores']

    def loss(self, xs, lengths, tags, domains, segments=None):
        """models/CRF.py:1141-1227."""
        if segments is not None:
            raise NotImplementedError('cosine auxiliary loss (models/CRF.py:23-92): no collater of the reference produces '
                                      "batch['src_segments'] (TextSegmenter.training_step raises KeyError upstream, fixture g15)")
        if torch.is_grad_enabled() and any(p.requires_grad for p in self._flat_params.values()):
            return self._autograd_loss(lambda: self.loss_and_grad(xs, lengths, tags, domains, True)[0])
        return self.loss_and_grad(xs, lengths, tags, domains, False)[0].clone()

    def forward(self, xs, lengths, domains, threshold=0.4):
        """models/CRF.py:1229-1270."""
        L.require_gpu()
        with torch.no_grad():
            st = self._fwd(xs, lengths, domains)
            scores = st['scores'].clone()
            tags = self._decode(scores, st['li32'], lengths, threshold)
        return scores, tags
