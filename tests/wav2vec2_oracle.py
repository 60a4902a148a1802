"""A torch restatement of the wav2vec 2.0 forward pass (``Wav2Vec2Model(...).last_hidden_state`` behind ``Wav2Vec2FeatureExtractor``'s
utterance normalisation), one sentence at a time, from a plain state dict -- the yardstick of tests/test_wav2vec2_cpu.py (where it is
itself checked against ``transformers``) and tests/test_gpu_wav2vec2.py.  Only the base configuration's structure is restated: group norm
on conv layer 0, no conv bias, exact (erf) GELU, the weight-normed grouped positional convolution with its dropped last frame, post-LN
transformer layers, no dropout.

``Oracle(sd, cfg, mode)`` runs in fp64 (``mode='fp64'``: the reference), in fp32 (``'fp32'``), or in fp32 with the matrices and every
STORED activation rounded to bf16 (``'bf16'``: what a bf16 device pass stores; the vectors -- biases, norm parameters, conv layer 0 -- stay
fp32 there as on the device).  The last two give ``e_ref`` of the tests' tolerance rule.  ``random_state_dict`` builds weights for a size
without importing ``transformers``.
"""
import math

import torch
import torch.nn.functional as F

SMALL = dict(conv_dim=32, kernels=(10, 3, 3, 3, 3, 2, 2), strides=(5, 2, 2, 2, 2, 2, 2), hidden=128, heads=4, intermediate=256, layers=2,
             pos_kernel=16, pos_groups=4, eps=1e-5)
BASE = dict(conv_dim=512, kernels=(10, 3, 3, 3, 3, 2, 2), strides=(5, 2, 2, 2, 2, 2, 2), hidden=768, heads=12, intermediate=3072, layers=12,
            pos_kernel=128, pos_groups=16, eps=1e-5)


def frame_count(n, cfg=BASE):
    for k, s in zip(cfg['kernels'], cfg['strides']):
        n = (n - k) // s + 1 if n >= k else 0
    return n


def hf_config_dict(cfg):
    """the part of a Wav2Vec2Config the tensors cannot tell, for ``Wav2Vec2Weights.from_state_dict``"""
    return {'num_attention_heads': cfg['heads'], 'conv_stride': cfg['strides'], 'num_conv_pos_embedding_groups': cfg['pos_groups'],
            'layer_norm_eps': cfg['eps']}


def random_state_dict(cfg, seed=0, spelling='weight_g'):
    """fp32 weights under Hugging Face's names: matrices N(0, 1 / fan_in) so that activations stay of order 1, norm scales 1 + 0.1 N,
    biases and shifts 0.1 N.  ``spelling``: 'weight_g' or 'parametrizations' for the positional convolution's weight norm."""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    C, H, I, Kp, G = cfg['conv_dim'], cfg['hidden'], cfg['intermediate'], cfg['pos_kernel'], cfg['pos_groups']
    sd, cin = {}, 1
    for i, k in enumerate(cfg['kernels']):
        sd[f'feature_extractor.conv_layers.{i}.conv.weight'] = rn(C, cin, k) * (1.5 / math.sqrt(cin * k))
        cin = C
    sd['feature_extractor.conv_layers.0.layer_norm.weight'] = 1 + 0.1 * rn(C)
    sd['feature_extractor.conv_layers.0.layer_norm.bias'] = 0.1 * rn(C)

    def norm(name, n):
        sd[name + '.weight'], sd[name + '.bias'] = 1 + 0.1 * rn(n), 0.1 * rn(n)

    def lin(name, o, i):
        sd[name + '.weight'], sd[name + '.bias'] = rn(o, i) / math.sqrt(i), 0.1 * rn(o)

    norm('feature_projection.layer_norm', C)
    lin('feature_projection.projection', H, C)
    sd['masked_spec_embed'] = rn(H)
    v = rn(H, H // G, Kp) / math.sqrt(Kp * H // G)
    gn = torch.sqrt((v.double() ** 2).sum(dim=(0, 1), keepdim=True)).float() * (1 + 0.1 * rn(1, 1, Kp))
    names = ('weight_g', 'weight_v') if spelling == 'weight_g' else ('parametrizations.weight.original0', 'parametrizations.weight.original1')
    sd['encoder.pos_conv_embed.conv.' + names[0]], sd['encoder.pos_conv_embed.conv.' + names[1]] = gn, v
    sd['encoder.pos_conv_embed.conv.bias'] = 0.1 * rn(H)
    norm('encoder.layer_norm', H)
    for i in range(cfg['layers']):
        p = f'encoder.layers.{i}.'
        for n in ('q_proj', 'k_proj', 'v_proj', 'out_proj'):
            lin(p + 'attention.' + n, H, H)
        norm(p + 'layer_norm', H)
        lin(p + 'feed_forward.intermediate_dense', I, H)
        lin(p + 'feed_forward.output_dense', H, I)
        norm(p + 'final_layer_norm', H)
    return sd


def signals(lengths, seed=0, offset_at=3):
    """seeded test sentences: white noise plus a sine; sentence ``offset_at`` carries a constant offset of 3.0"""
    g = torch.Generator().manual_seed(seed)
    out = []
    for i, n in enumerate(lengths):
        t = torch.arange(n, dtype=torch.float64)
        x = 0.3 * torch.randn(n, generator=g, dtype=torch.float64) + 0.5 * torch.sin(2 * math.pi * (110.0 + 37.0 * i) * t / 16000.0)
        out.append((x + (3.0 if i == offset_at else 0.0)).float())
    return out


def _bf16(t):
    return t.to(torch.bfloat16).to(t.dtype)


class Oracle:
    def __init__(self, sd, cfg, mode='fp64'):
        assert mode in ('fp64', 'fp32', 'bf16')
        self.cfg, self.mode = cfg, mode
        self.ct = torch.float64 if mode == 'fp64' else torch.float32
        self.ra = _bf16 if mode == 'bf16' else (lambda t: t)
        sd = {(k[len('wav2vec2.'):] if k.startswith('wav2vec2.') else k): v.detach().double() for k, v in sd.items()}
        pc = 'encoder.pos_conv_embed.conv.'
        gk, vk = (pc + 'weight_g', pc + 'weight_v') if pc + 'weight_g' in sd else (pc + 'parametrizations.weight.original0',
                                                                                  pc + 'parametrizations.weight.original1')
        v = sd[vk]
        sd[pc + 'weight'] = sd[gk].reshape(1, 1, -1) * v / torch.sqrt((v * v).sum(dim=(0, 1), keepdim=True))
        self.sd = sd

    def vec(self, name):
        return self.sd[name].to(self.ct)

    def mat(self, name):
        w = self.sd[name]
        return (w.float().to(torch.bfloat16).float() if self.mode == 'bf16' else w).to(self.ct)

    # ---- stages: each takes its input in any dtype and returns [frames, channels] in the compute dtype -------------------------------
    def wave_stats(self, x):
        x = x.to(self.ct)
        return x.mean(), 1.0 / torch.sqrt(x.var(unbiased=False) + 1e-7)

    def conv0(self, x):
        x = x.to(self.ct)
        mean, rstd = self.wave_stats(x)
        c = F.conv1d(((x - mean) * rstd)[None, None], self.vec('feature_extractor.conv_layers.0.conv.weight'), stride=self.cfg['strides'][0])[0]
        m, v = c.mean(dim=1, keepdim=True), c.var(dim=1, unbiased=False, keepdim=True)
        y = (c - m) / torch.sqrt(v + 1e-5) * self.vec('feature_extractor.conv_layers.0.layer_norm.weight')[:, None] \
            + self.vec('feature_extractor.conv_layers.0.layer_norm.bias')[:, None]
        return self.ra(F.gelu(y).t().contiguous())

    def conv(self, layer, x):
        c = F.conv1d(x.to(self.ct).t()[None], self.mat(f'feature_extractor.conv_layers.{layer}.conv.weight'), stride=self.cfg['strides'][layer])[0]
        return self.ra(F.gelu(c).t().contiguous())

    def _ln(self, x, name):
        return self.ra(F.layer_norm(x, (x.shape[-1],), self.vec(name + '.weight'), self.vec(name + '.bias'), self.cfg['eps']))

    def _lin(self, x, name):
        return x @ self.mat(name + '.weight').t() + self.vec(name + '.bias')

    def project(self, x):
        return self.ra(self._lin(self._ln(x.to(self.ct), 'feature_projection.layer_norm'), 'feature_projection.projection'))

    def pos_conv(self, h):
        h = h.to(self.ct)
        Kp = self.cfg['pos_kernel']
        c = F.conv1d(h.t()[None], self.mat('encoder.pos_conv_embed.conv.weight'), self.vec('encoder.pos_conv_embed.conv.bias'), padding=Kp // 2,
                     groups=self.cfg['pos_groups'])[0]
        if Kp % 2 == 0:
            c = c[:, :-1]
        return self.ra(h + F.gelu(c).t())

    def encoder(self, y, layers=None):
        H, heads = self.cfg['hidden'], self.cfg['heads']
        hd = H // heads
        x = self._ln(y.to(self.ct), 'encoder.layer_norm')
        for i in range(self.cfg['layers'] if layers is None else layers):
            p = f'encoder.layers.{i}.'
            q = self.ra(self._lin(x, p + 'attention.q_proj') * hd ** -0.5)
            k, v = self.ra(self._lin(x, p + 'attention.k_proj')), self.ra(self._lin(x, p + 'attention.v_proj'))
            T = x.shape[0]
            q, k, v = (t.view(T, heads, hd).transpose(0, 1) for t in (q, k, v))
            ctx = self.ra((torch.softmax(q @ k.transpose(1, 2), dim=-1) @ v).transpose(0, 1).reshape(T, H))
            a1 = self._ln(self.ra(x + self._lin(ctx, p + 'attention.out_proj')), p + 'layer_norm')
            u = self.ra(F.gelu(self._lin(a1, p + 'feed_forward.intermediate_dense')))
            x = self._ln(self.ra(a1 + self._lin(u, p + 'feed_forward.output_dense')), p + 'final_layer_norm')
        return x

    def features(self, x):
        y = self.conv0(x)
        for l in range(1, len(self.cfg['kernels'])):
            y = self.conv(l, y)
        return y

    def forward(self, x):
        """raw samples [n] -> last_hidden_state [frames, hidden]"""
        return self.encoder(self.pos_conv(self.project(self.features(x))))


def within(dev, oracle, ref, eps, what=''):
    """the tests' tolerance rule: e_dev <= 4 e_ref + 4 eps max|oracle|; prints the figures before asserting -> e_dev / bound"""
    e_dev = float((dev.double() - oracle.double()).abs().max())
    e_ref = float((ref.double() - oracle.double()).abs().max())
    bound = 4.0 * e_ref + 4.0 * eps * float(oracle.abs().max())
    print(f'{what}: e_dev={e_dev:.3e} e_ref={e_ref:.3e} max|oracle|={float(oracle.abs().max()):.3e} bound={bound:.3e} ratio={e_dev / bound:.3f}')
    assert e_dev <= bound, (what, e_dev, e_ref, bound)
    return e_dev / bound
