"""wav2vec 2.0 sentence features from resident waveforms: the reference's learned audio encoder on the device.

extract_embeddings.py:173-183 (``--wav2vec``) runs, per sentence, ``Wav2Vec2Processor`` (zero mean, unit variance) and
``Wav2Vec2Model(...).last_hidden_state`` ([frames, 768]) at batch size 1, writes the frames to ``_no_reduction/<file>.pkl`` and pools them
six ways (:609-667).  ``ResidentAudio.wav2vec2(weights)`` (audio.py) makes the same frames in HBM for a whole corpus, a chunk of sentences
at a time, as a ``frames.ResidentFrames`` that ``pool(mode)`` and ``ResidentCorpus.with_frames`` take unchanged.  Inference only.

``Wav2Vec2Weights.from_state_dict`` lays a Hugging Face ``Wav2Vec2Model`` state dict out for the kernels; this module composes the forward
pass of a chunk, as the taggers compose theirs, from csrc/wav2vec2.hip and the GEMM, LayerNorm and full-attention entry points:

  * activations are time-major [rows, channels] in the chosen dtype (fp32: the parity mode; bf16: the fast mode);
  * sentence s owns a block of layer-0 rows that starts at a multiple of 64, so its block at conv layer l starts at ``base >> l`` and
    conv layers 1 .. 6 (stride 2, kernel k, C_in = C_out = C) are ONE NT GEMM each over the whole chunk: output row t is the product of
    the overlapping row A = x + 2 t C (lda = 2 C, K = k C) with the weights permuted to [C_out, k * C_in], GELU epilogue.  Rows between
    blocks are computed and never read as valid rows: a valid output row reads only rows of its own sentence (the length formula);
  * layer 0 (C_in = 1) is two launches: the GroupNorm statistics of the conv output (never stored) and the recompute;
  * the positional convolution is ``ops.w2v_pos_conv`` (bf16, matrix cores) or its GEMM form: ``ops.w2v_regroup`` writes the chunk
    group-major with K_p / 2 zero rows in front of every sentence, one overlapping-row GEMM per group (lda = H / G, K = K_p H / G) writes
    gelu(conv + bias) into its column block, and ``ops.w2v_rows`` compacts the valid rows and adds the residual;
  * the transformer runs on the compact [frames, H] rows: ``lengths`` / ``row0`` keep every sentence an independent sequence.
"""
import numpy as np
import torch

ACT_DTYPES = {'fp32': torch.float32, 'bf16': torch.bfloat16}
ALIGN = 64                                  # layer-0 rows a sentence's block is aligned to: 2^6 for the six stride-2 layers
SLACK = 8                                   # rows behind a conv buffer that the overlapping reads of its last rows reach (k - 2 <= 8)
DEFAULT_STRIDES = (5, 2, 2, 2, 2, 2, 2)
_IGNORED = ('masked_spec_embed', 'adapter.', 'quantizer.', 'project_q.', 'project_hid.', 'lm_head.', 'classifier.', 'projector.',
            'feature_extractor_head.', 'tdnn.', 'objective.', 'layer_weights')


def cfg_get(config, name, default=None):
    if config is None:
        return default
    if isinstance(config, dict):
        return config.get(name, default)
    return getattr(config, name, default)


def frame_counts(n, kernels, strides):
    """frames the conv chain gives for n samples: T <- (T - k) // stride + 1 through the layers, 0 once a layer has fewer than k inputs"""
    T = np.asarray(n, dtype=np.int64).copy()
    for k, st in zip(kernels, strides):
        T = np.where(T >= k, (T - k) // st + 1, 0)
    return T


def effective_pos_weight(g, v):
    """weight norm of the positional convolution as HF applies it (``dim=2``): w = g * v / ||v||, the norm over dims (0, 1) per tap; formed
    in fp64 -> fp64 [H, H / G, K_p]"""
    v = v.detach().to(torch.float64)
    g = g.detach().to(torch.float64).reshape(1, 1, -1)
    return g * v / torch.sqrt((v * v).sum(dim=(0, 1), keepdim=True))


class Wav2Vec2Weights:
    """The parameters of a Hugging Face ``Wav2Vec2Model`` laid out once for the kernels (use ``from_state_dict``).

    Host attributes: ``conv_dim`` C, ``hidden_size`` H, ``intermediate_size``, ``num_layers``, ``num_heads``, ``kernels``, ``strides``,
    ``pos_kernel`` K_p, ``pos_groups`` G, ``eps``, ``dtype`` (torch.float32 | torch.bfloat16), ``device``.  Tensors on ``device``: fp32
    ``conv0_w`` [C, k_0], ``gn_gamma`` / ``gn_beta`` [C]; in ``dtype`` ``conv_w[l - 1]`` [C, k_l * C] (l = 1 ..: [C_out, C_in, k] permuted to
    [C_out, k * C_in]), ``proj_w`` [H, C], ``pos_w`` [G, H / G, K_p * H / G] (the effective weight, [out, in, tap] permuted to [out, tap *
    in] per group), per layer ``qkv_w`` [3 H, H] (q | k | v), ``o_w``, ``ff1_w``, ``ff2_w``; fp32 biases and LayerNorm parameters."""

    @classmethod
    def from_state_dict(cls, sd, config=None, device='cpu', dtype='bf16'):
        if dtype not in ACT_DTYPES:
            raise ValueError("Wav2Vec2Weights: dtype must be 'bf16' or 'fp32'")
        src = {}
        for k, t in sd.items():
            k = k[len('wav2vec2.'):] if k.startswith('wav2vec2.') else k
            if k.startswith(_IGNORED):
                continue
            src[k] = t.detach().to('cpu', torch.float32).contiguous()
        self = cls.__new__(cls)
        self.dtype, self.device = ACT_DTYPES[dtype], torch.device(device)
        if self.device.type == 'cuda' and self.device.index is None:
            self.device = torch.device('cuda', torch.cuda.current_device())
        fe ='feature_extractor.conv_layers.'
        n_conv = 0
        while f'{fe}{n_conv}.conv.weight' in src:
            n_conv += 1
        if n_conv < 2:
            raise ValueError('Wav2Vec2Weights: the state dict holds no feature_extractor.conv_layers.*.conv.weight')
        if any(f'{fe}{i}.conv.bias' in src for i in range(n_conv)):
            raise NotImplementedError('Wav2Vec2Weights: conv_bias=True (conv biases present); only conv_bias=False is supported')
        if any(f'{fe}{i}.layer_norm.weight' in src for i in range(1, n_conv)) or cfg_get(config, 'feat_extract_norm', 'group') != 'group':
            raise NotImplementedError("Wav2Vec2Weights: feat_extract_norm='layer' (a layer norm in every conv layer); only 'group' is supported")
        if f'{fe}0.layer_norm.weight' not in src:
            raise NotImplementedError("Wav2Vec2Weights: no group norm on conv layer 0; only feat_extract_norm='group' is supported")
        if cfg_get(config, 'do_stable_layer_norm', False):
            raise NotImplementedError('Wav2Vec2Weights: do_stable_layer_norm=True; only the post-LayerNorm encoder is supported')
        for name in ('feat_extract_activation', 'hidden_act'):
            if cfg_get(config, name, 'gelu') != 'gelu':
                raise NotImplementedError(f"Wav2Vec2Weights: {name}={cfg_get(config, name)!r}; only 'gelu' is supported")
        convs = [src[f'{fe}{i}.conv.weight'] for i in range(n_conv)]
        self.kernels = tuple(int(w.shape[2]) for w in convs)
        strides = cfg_get(config, 'conv_stride', DEFAULT_STRIDES)
        self.strides = tuple(int(s) for s in strides)
        C = self.conv_dim = int(convs[0].shape[0])
        if len(self.strides) != n_conv:
            raise ValueError(f'Wav2Vec2Weights: conv_stride has {len(self.strides)} entries for {n_conv} conv layers')
        if (int(convs[0].shape[1]) != 1 or n_conv > 7 or any(s != 2 for s in self.strides[1:]) or any(tuple(w.shape[:2]) != (C, C) for w in convs[1:])
                or any(not 2 <= k <= 2 + SLACK for k in self.kernels[1:])):
            raise NotImplementedError(f'Wav2Vec2Weights: conv layers {[tuple(w.shape) for w in convs]} with strides {self.strides}: one input channel, at '
                                      'most seven layers of one width, stride 2 and kernels 2 .. 10 behind the first are supported')
        pc = 'encoder.pos_conv_embed.conv.'
        spell = [(pc + 'weight_g', pc + 'weight_v'), (pc + 'parametrizations.weight.original0', pc + 'parametrizations.weight.original1')]
        found = [p for p in spell if p[0] in src and p[1] in src]
        if not found:
            raise ValueError('Wav2Vec2Weights: the positional convolution has neither weight_g / weight_v nor parametrizations.weight.original0 / 1')
        self._pos_g, self._pos_v = src[found[0][0]], src[found[0][1]]
        H, cg, Kp = (int(d) for d in self._pos_v.shape)
        self.hidden_size, self.pos_kernel = H, Kp
        self.pos_groups = int(cfg_get(config, 'num_conv_pos_embedding_groups', 16))
        if Kp % 2:
            raise NotImplementedError(f'Wav2Vec2Weights: an odd positional kernel ({Kp}); only even kernels (which drop their last frame) are supported')
        if cg * self.pos_groups != H:
            raise ValueError(f'Wav2Vec2Weights: positional weight {tuple(self._pos_v.shape)} does not fit {self.pos_groups} groups of hidden size {H}')
        self.eps = float(cfg_get(config, 'layer_norm_eps', 1e-5))
        L = 0
        while f'encoder.layers.{L}.attention.q_proj.weight' in src:
            L += 1
        self.num_layers = L
        self.num_heads = int(cfg_get(config, 'num_attention_heads', max(H // 64, 1)))
        if H % self.num_heads:
            raise ValueError(f'Wav2Vec2Weights: hidden size {H} is not divisible by {self.num_heads} heads')
        self.intermediate_size = int(src['encoder.layers.0.feed_forward.intermediate_dense.weight'].shape[0]) if L else 0
        self._src = {k: v for k, v in src.items() if k not in spell[0] + spell[1]}

        act = lambda t: t.to(self.dtype).contiguous().to(self.device)
        f32 = lambda t: t.to(torch.float32).contiguous().to(self.device)
        self.conv0_w = f32(convs[0].reshape(C, self.kernels[0]))
        self.gn_gamma, self.gn_beta = f32(src[f'{fe}0.layer_norm.weight']), f32(src[f'{fe}0.layer_norm.bias'])
        self.conv_w = [act(w.permute(0, 2, 1).reshape(C, -1)) for w in convs[1:]]
        self.fp_gamma, self.fp_beta = f32(src['feature_projection.layer_norm.weight']), f32(src['feature_projection.layer_norm.bias'])
        self.proj_w, self.proj_b = act(src['feature_projection.projection.weight']), f32(src['feature_projection.projection.bias'])
        w_eff = effective_pos_weight(self._pos_g, self._pos_v)                                  # fp64, rounded once below
        self.pos_w = act(w_eff.permute(0, 2, 1).reshape(self.pos_groups, cg, Kp * cg).to(torch.float32))
        self.pos_b = f32(src[pc + 'bias'])
        self.enc_gamma, self.enc_beta = f32(src['encoder.layer_norm.weight']), f32(src['encoder.layer_norm.bias'])
        self.layers = []
        for i in range(L):
            p = f'encoder.layers.{i}.'
            a = p + 'attention.'
            self.layers.append({
                'qkv_w': act(torch.cat([src[a + f'{n}_proj.weight'] for n in 'qkv'])), 'qkv_b': f32(torch.cat([src[a + f'{n}_proj.bias'] for n in 'qkv'])),
                'o_w': act(src[a + 'out_proj.weight']), 'o_b': f32(src[a + 'out_proj.bias']),
                'ln1_g': f32(src[p + 'layer_norm.weight']), 'ln1_b': f32(src[p + 'layer_norm.bias']),
                'ff1_w': act(src[p + 'feed_forward.intermediate_dense.weight']), 'ff1_b': f32(src[p + 'feed_forward.intermediate_dense.bias']),
                'ff2_w': act(src[p + 'feed_forward.output_dense.weight']), 'ff2_b': f32(src[p + 'feed_forward.output_dense.bias']),
                'ln2_g': f32(src[p + 'final_layer_norm.weight']), 'ln2_b': f32(src[p + 'final_layer_norm.bias'])})
        return self

    def state_dict(self):
        """-> the fp32 host tensors ``from_state_dict`` took, under Hugging Face's names without a prefix (the weight norm as ``weight_g`` /
        ``weight_v``): ``from_state_dict(w.state_dict(), config)`` gives the same weights"""
        out = dict(self._src)
        out['encoder.pos_conv_embed.conv.weight_g'] = self._pos_g
        out['encoder.pos_conv_embed.conv.weight_v'] = self._pos_v
        return out

    def config(self):
        """what the tensors cannot tell, as a dict ``from_state_dict`` takes"""
        return {'num_attention_heads': self.num_heads, 'conv_stride': self.strides, 'num_conv_pos_embedding_groups': self.pos_groups,
                'layer_norm_eps': self.eps}

    @property
    def min_samples(self):
        """the fewest samples that give a frame (400 at the default kernels and strides)"""
        n = 1
        for k, s in zip(reversed(self.kernels), reversed(self.strides)):
            n = (n - 1) * s + k
        return n


class ChunkPlan:
    """Where every sentence of a chunk lives (host arithmetic; the tables go to the device once per chunk).  ``T`` [n_layers, n_sent] frames
    per conv layer; ``block_start`` [n_sent + 1] layer-0 row blocks in multiples of 64 (``rows0`` = its last entry; the block at layer l
    starts at ``block_start >> l``); ``frame_start`` [n_sent + 1] the compact output rows; ``pad_start`` [n_sent + 1] the padded rows of
    the GEMM form of the positional convolution; ``tile_start`` [n_sent + 1] 64-frame tiles."""

    def __init__(self, sample_counts, weights, device=None):
        n = np.asarray(sample_counts, dtype=np.int64)
        T, layers = n.copy(), []
        for k, st in zip(weights.kernels, weights.strides):
            T = np.where(T >= k, (T - k) // st + 1, 0)
            layers.append(T)
        self.T = np.stack(layers)
        self.n_sent, self.n_layers = int(n.size), len(layers)
        self.frames = self.T[-1]
        cum = lambda a: np.concatenate([[0], np.cumsum(a)]).astype(np.int64)
        self.block_start = cum((np.maximum(self.T[0], 1) + ALIGN - 1) // ALIGN * ALIGN)
        self.rows0 = int(self.block_start[-1])
        self.frame_start = cum(self.frames)
        self.total_frames = int(self.frame_start[-1])
        self.pad_start = cum(self.frames + weights.pos_kernel // 2)
        self.rows_p = int(self.pad_start[-1]) + weights.pos_kernel
        self.tile_start = cum((self.frames + 63) // 64).astype(np.int32)
        self.max_frames = int(self.frames.max())
        self.dev = {}
        if device is not None and torch.device(device).type == 'cuda':
            up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
            last = self.n_layers - 1
            self.dev = {'block_start': up(self.block_start), 'frame_start': up(self.frame_start), 'pad_start': up(self.pad_start),
                        'tile_start': up(self.tile_start), 'top_row0': up(self.block_start[:-1] >> last), 'pad_row0': up(self.pad_start[:-1]),
                        'frame_row0': up(self.frame_start[:-1]), 'row0_i32': up(self.frame_start[:-1].astype(np.int32)),
                        'lengths_i32': up(self.frames.astype(np.int32))}

    def valid_rows(self, buf, layer):
        """the sentences' own rows of a conv-layer buffer, one after another -> [sum T_layer, C]"""
        return torch.cat([buf[int(b) >> layer:(int(b) >> layer) + int(t)] for b, t in zip(self.block_start[:-1], self.T[layer])])


def conv_layer0(w, wave, sent_start, sent_len, plan, out=None):
    """utterance normalisation + conv layer 0 + GroupNorm + GELU of a chunk -> (x0 [rows0 + SLACK, C], wave_stats, gmean, grstd)"""
    from . import ops
    stats = ops.w2v_wave_stats(wave, sent_start, sent_len)
    gmean, grstd = ops.w2v_conv0_stats(wave, sent_start, sent_len, stats, w.conv0_w, w.strides[0], 1e-5)
    if out is None:
        out = torch.empty((plan.rows0 + SLACK, w.conv_dim), dtype=w.dtype, device=wave.device)
    out[plan.rows0:].zero_()
    ops.w2v_conv0(wave, sent_start, sent_len, stats, w.conv0_w, w.strides[0], gmean, grstd, w.gn_gamma, w.gn_beta, plan.dev['block_start'], plan.rows0, out)
    return out, stats, gmean, grstd


def conv_gemm(w, layer, x, rows_in, out=None):
    """conv layer ``layer`` >= 1 over a whole chunk as ONE overlapping-row NT GEMM: x [>= rows_in + k - 2, C] -> out [rows_in / 2 (+ SLACK), C]"""
    from . import ops
    from . import _lib as L
    C, k, M = w.conv_dim, w.kernels[layer], rows_in // 2
    assert int(x.shape[0]) >= rows_in + k - 2 and x.is_contiguous()
    if out is None:
        out = torch.empty((M + SLACK, C), dtype=w.dtype, device=x.device)
        out[M:].zero_()
    ops.gemm(L.NT, x, w.conv_w[layer - 1], out, M=M, N=C, K=k * C, lda=2 * C, ldb=k * C, ldc=C, gelu=True)
    return out


def conv_features(w, wave, sent_start, sent_len, plan, keep=False):
    """the seven conv layers of a chunk -> the last layer's buffer (sentence s at rows ``block_start[s] >> 6``), or with ``keep`` the list
    of every layer's buffer (the tests' stage-by-stage view).  Without ``keep`` two buffers alternate: layer 0's and layer 1's."""
    x0 = conv_layer0(w, wave, sent_start, sent_len, plan)[0]
    bufs, rows = [x0], plan.rows0
    for l in range(1, plan.n_layers):
        reuse = None if keep or l < 2 else bufs[l - 2]
        bufs.append(conv_gemm(w, l, bufs[-1], rows, out=reuse))
        rows //= 2
    return bufs if keep else bufs[-1]


def project(w, top, plan):
    """the feature projection: LayerNorm at D = conv_dim, then one GEMM with bias -> h [rows_top, H] (sentence s at ``top_row0[s]``)"""
    from . import ops
    R = plan.rows0 >> (plan.n_layers - 1)
    x = top[:R]
    y = torch.empty_like(x)
    mean, rstd = (torch.empty(R, dtype=torch.float32, device=x.device) for _ in range(2))
    ops.layernorm_fwd(x, w.fp_gamma, w.fp_beta, w.eps, y, mean, rstd)
    h = torch.empty((R, w.hidden_size), dtype=w.dtype, device=x.device)
    return ops.linear_fwd(y, w.proj_w, w.proj_b, h)


def pos_conv_gemm(w, h, plan, keep=False):
    """y = x + gelu(pos_conv(x)) in its GEMM form -> compact [total_frames, H] (with ``keep`` also the regrouped buffer)"""
    from . import ops
    from . import _lib as L
    H, G, Kp = w.hidden_size, w.pos_groups, w.pos_kernel
    cg = H // G
    xg = ops.w2v_regroup(h, plan.dev['top_row0'], plan.dev['pad_start'], plan.rows_p, G, Kp)
    M = int(plan.pad_start[-1])
    conv = torch.empty((M, H), dtype=w.dtype, device=h.device)
    for g in range(G):
        ops.gemm(L.NT, xg[g], w.pos_w[g], conv[:, g * cg:(g + 1) * cg], M=M, N=cg, K=Kp * cg, lda=cg, ldb=Kp * cg, ldc=H,
                 bias=w.pos_b[g * cg:(g + 1) * cg], gelu=True)
    y = torch.empty((plan.total_frames, H), dtype=w.dtype, device=h.device)
    ops.w2v_rows(conv, plan.dev['pad_row0'], plan.dev['frame_start'], y, res=h, res_row0=plan.dev['top_row0'])
    return (y, xg) if keep else y


def pos_conv_kernel(w, h, plan):
    """the same on the matrix cores (bf16 weights only) -> compact [total_frames, H]"""
    from . import ops
    y = torch.empty((plan.total_frames, w.hidden_size), dtype=w.dtype, device=h.device)
    return ops.w2v_pos_conv(h, plan.dev['top_row0'], plan.dev['frame_start'], plan.dev['tile_start'], int(plan.tile_start[-1]), w.pos_w, w.pos_b,
                            w.pos_groups, w.pos_kernel, y)


def pos_conv_kernel_covers(w):
    cg = w.hidden_size // w.pos_groups
    return w.dtype == torch.bfloat16 and cg <= 64 and (w.pos_kernel * cg) % 128 == 0


def encoder_layers(layers, cur, lengths, row0, n_seq, max_len, heads, eps, out=None, attn='full'):
    """post-LN transformer layers on compact rows, shared by the wav2vec 2.0 encoder and the text encoder (text.py): ``cur`` [F, H] is the
    input and the buffer the layers but the last write back to; ``lengths`` / ``row0`` (int32 [n_seq], on the device) keep every
    sequence a sequence of its own.  ``layers``: dicts of qkv_w [3 H, H] (q | k | v), o_w, ff1_w, ff2_w in the activations' dtype and the
    fp32 biases and LayerNorm parameters.  ``attn``: 'full' (mts_full_attn_fwd) or 'sentence' (mts_sent_attn_fwd).  -> the last
    LayerNorm's output (``out`` if given)"""
    from . import ops
    n = len(layers)
    if n == 0:
        return cur
    F, H = (int(d) for d in cur.shape)
    I = int(layers[0]['ff1_w'].shape[0])
    new = lambda *shape: torch.empty(shape, dtype=cur.dtype, device=cur.device)
    mean, rstd = (torch.empty(F, dtype=torch.float32, device=cur.device) for _ in range(2))
    qkv, ctx, s1, a1, u, s2 = new(F, 3 * H), new(F, H), new(F, H), new(F, H), new(F, I), new(F, H)
    lse = torch.empty((F, heads), dtype=torch.float32, device=cur.device) if attn == 'full' else None
    for i, p in enumerate(layers):
        ops.linear_fwd(cur, p['qkv_w'], p['qkv_b'], qkv, colscale=float(H // heads) ** -0.5, ncols_scaled=H)
        if attn == 'full':
            ops.full_attn_fwd(qkv, lengths, n_seq, max_len, H, heads, ctx, lse, row0=row0)
        else:
            ops.sent_attn_fwd(qkv, row0, lengths, max_len, H, heads, ctx)
        ops.linear_fwd(ctx, p['o_w'], p['o_b'], s1, residual=cur)
        ops.layernorm_fwd(s1, p['ln1_g'], p['ln1_b'], eps, a1, mean, rstd)
        ops.linear_fwd(a1, p['ff1_w'], p['ff1_b'], u, gelu=True)
        ops.linear_fwd(u, p['ff2_w'], p['ff2_b'], s2, residual=a1)
        dst = out if (i == n - 1 and out is not None) else cur
        ops.layernorm_fwd(s2, p['ln2_g'], p['ln2_b'], eps, dst, mean, rstd)
        cur = dst
    return cur


def transformer(w, x, plan, out=None):
    """the encoder's LayerNorm and its post-LN layers on compact rows x [F, H] -> [F, H] (``out``: where the last LayerNorm writes)"""
    from . import ops
    F, H = plan.total_frames, w.hidden_size
    mean, rstd = (torch.empty(F, dtype=torch.float32, device=x.device) for _ in range(2))
    n = len(w.layers)
    cur = out if (n == 0 and out is not None) else torch.empty((F, H), dtype=w.dtype, device=x.device)
    ops.layernorm_fwd(x, w.enc_gamma, w.enc_beta, w.eps, cur, mean, rstd)
    return encoder_layers(w.layers, cur, plan.dev['lengths_i32'], plan.dev['row0_i32'], plan.n_sent, plan.max_frames, w.num_heads, w.eps, out=out)


def forward_chunk(w, wave, sent_start, sent_len, plan, out, pos='auto'):
    """the whole pass of one chunk of sentences into ``out`` [total_frames, H] (fp32 / bf16, contiguous).  ``pos``: 'kernel' | 'gemm' |
    'auto' (the kernel where it covers the shape and the weights are bf16)"""
    from . import ops
    top = conv_features(w, wave, sent_start, sent_len, plan)
    h = project(w, top, plan)
    del top
    if pos not in ('auto', 'kernel', 'gemm'):
        raise ValueError("pos is 'auto', 'kernel' or 'gemm'")
    use_kernel = pos == 'kernel' or (pos == 'auto' and pos_conv_kernel_covers(w))
    x = pos_conv_kernel(w, h, plan) if use_kernel else pos_conv_gemm(w, h, plan)
    del h
    if out.dtype == w.dtype:
        transformer(w, x, plan, out=out)
    else:
        y = transformer(w, x, plan)
        ops.w2v_rows(y, plan.dev['frame_row0'], plan.dev['frame_start'], out)
    return out


def chunk_bytes(w, sample_counts):
    """an upper estimate of the device bytes the pass of each sentence takes -> int64 [n]: its layer-0 block in the two alternating conv
    buffers, and per frame the projection, the padded positional buffers and the transformer's activations"""
    e = 2 if w.dtype == torch.bfloat16 else 4
    n = np.asarray(sample_counts, dtype=np.int64)
    T0 = frame_counts(n, w.kernels[:1], w.strides[:1])
    T = frame_counts(n, w.kernels, w.strides)
    rows0 = (np.maximum(T0, 1) + ALIGN - 1) // ALIGN * ALIGN
    per_frame = e * (2 * w.conv_dim + 12 * w.hidden_size + w.intermediate_size) + 4 * (w.num_heads + 2)
    return rows0 * (w.conv_dim * e * 3 // 2) + (T + w.pos_kernel) * per_frame + 8 * w.conv_dim
