"""A torch restatement of a BERT-family encoder (``BertModel`` / ``RobertaModel`` / ``XLMRobertaModel`` ``last_hidden_state``), one
sentence at a time, from a plain state dict -- the yardstick of tests/test_text_encoder_cpu.py (where it is itself checked against
``transformers``) and tests/test_gpu_text_encoder.py.  Only the covered structure is restated: absolute position embeddings (from
``offset``: 2 for the RoBERTa family, 0 for BERT), token type 0, exact (erf) GELU, post-LN layers, no dropout.

``Oracle(sd, cfg, mode)`` runs in fp64 (``mode='fp64'``: the reference), in fp32 (``'fp32'``), or in fp32 with the matrices, the embedding
tables and every STORED activation rounded to bf16 (``'bf16'``: what a bf16 device pass stores; biases and norm parameters stay fp32 there
as on the device).  The last two give ``e_ref`` of the tests' tolerance rule (``within``, shared with the wav2vec 2.0 tests).
``random_state_dict`` builds weights for a size without importing ``transformers``.
"""
import math

import torch
import torch.nn.functional as F

from tests.wav2vec2_oracle import _bf16, within  # noqa: F401  (within: the tests' tolerance rule)

TINY = dict(vocab=97, hidden=64, heads=2, intermediate=128, layers=2, positions=40, eps=1e-12)
REAL = dict(vocab=1000, hidden=768, heads=12, intermediate=3072, layers=2, positions=80, eps=1e-12)
OFFSET = {'bert': 0, 'roberta': 2, 'xlm-roberta': 2}
EPS = {'fp32': 2.0 ** -23, 'bf16': 2.0 ** -7}


def config_dict(cfg, family):
    """what the tensors cannot tell, for ``TextEncoderWeights.from_state_dict``, as a Hugging Face config spells it"""
    return {'model_type': family, 'pad_token_id': 0 if family == 'bert' else 1, 'num_attention_heads': cfg['heads'], 'layer_norm_eps': cfg['eps'],
            'hidden_act': 'gelu'}


def random_state_dict(cfg, seed=0):
    """fp32 weights under Hugging Face's names: matrices N(0, 1 / fan_in), embedding tables N(0, 1), norm scales 1 + 0.1 N, biases and
    shifts 0.1 N; two token types as BERT has (only row 0 is used)"""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    H, I = cfg['hidden'], cfg['intermediate']
    sd = {'embeddings.word_embeddings.weight': rn(cfg['vocab'], H), 'embeddings.position_embeddings.weight': rn(cfg['positions'], H),
          'embeddings.token_type_embeddings.weight': rn(2, H)}

    def norm(name):
        sd[name + '.weight'], sd[name + '.bias'] = 1 + 0.1 * rn(H), 0.1 * rn(H)

    def lin(name, o, i):
        sd[name + '.weight'], sd[name + '.bias'] = rn(o, i) / math.sqrt(i), 0.1 * rn(o)

    norm('embeddings.LayerNorm')
    for i in range(cfg['layers']):
        p = f'encoder.layer.{i}.'
        for n in ('query', 'key', 'value'):
            lin(p + 'attention.self.' + n, H, H)
        lin(p + 'attention.output.dense', H, H)
        norm(p + 'attention.output.LayerNorm')
        lin(p + 'intermediate.dense', I, H)
        lin(p + 'output.dense', H, I)
        norm(p + 'output.LayerNorm')
    return sd


def sentences(lengths, vocab, seed=0):
    """seeded id sequences; the first holds the vocabulary's first and last id"""
    g = torch.Generator().manual_seed(seed)
    out = [torch.randint(0, vocab, (n,), generator=g) for n in lengths]
    out[0][0] = vocab - 1
    out[0][-1] = 0
    return out


def attention(qkv, lengths, row0, heads, ct=torch.float64):
    """softmax attention of packed sequences on a [rows, 3 D] matrix with q already scaled -> ctx [rows, D] in ``ct``; rows outside the
    listed sequences stay 0"""
    D = qkv.shape[1] // 3
    hd = D // heads
    ctx = torch.zeros((qkv.shape[0], D), dtype=ct)
    for r, n in zip(row0, lengths):
        q, k, v = (qkv[r:r + n, i * D:(i + 1) * D].to(ct).view(n, heads, hd).transpose(0, 1) for i in range(3))
        ctx[r:r + n] = (torch.softmax(q @ k.transpose(1, 2), dim=-1) @ v).transpose(0, 1).reshape(n, D)
    return ctx


class Oracle:
    def __init__(self, sd, cfg, mode='fp64', offset=0):
        assert mode in ('fp64', 'fp32', 'bf16')
        self.cfg, self.mode, self.offset = cfg, mode, offset
        self.ct = torch.float64 if mode == 'fp64' else torch.float32
        self.ra = _bf16 if mode == 'bf16' else (lambda t: t)
        self.sd = {k: v.detach().double() for k, v in sd.items()}

    def vec(self, name):
        return self.sd[name].to(self.ct)

    def mat(self, name):
        w = self.sd[name]
        return (w.float().to(torch.bfloat16).float() if self.mode == 'bf16' else w).to(self.ct)

    def _ln(self, x, name):
        return self.ra(F.layer_norm(x, (x.shape[-1],), self.vec(name + '.weight'), self.vec(name + '.bias'), self.cfg['eps']))

    def _lin(self, x, name):
        return x @ self.mat(name + '.weight').t() + self.vec(name + '.bias')

    def embed(self, ids):
        e = 'embeddings.'
        pos = torch.arange(len(ids)) + self.offset
        x = (self.mat(e + 'word_embeddings.weight')[ids] + self.mat(e + 'position_embeddings.weight')[pos]) + self.mat(e + 'token_type_embeddings.weight')[0]
        return self._ln(x, e + 'LayerNorm')

    def layer(self, x, i):
        H, heads = self.cfg['hidden'], self.cfg['heads']
        hd, T = H // heads, x.shape[0]
        p = f'encoder.layer.{i}.'
        q = self.ra(self._lin(x, p + 'attention.self.query') * hd ** -0.5)
        k, v = self.ra(self._lin(x, p + 'attention.self.key')), self.ra(self._lin(x, p + 'attention.self.value'))
        q, k, v = (t.view(T, heads, hd).transpose(0, 1) for t in (q, k, v))
        ctx = self.ra((torch.softmax(q @ k.transpose(1, 2), dim=-1) @ v).transpose(0, 1).reshape(T, H))
        a1 = self._ln(self.ra(x + self._lin(ctx, p + 'attention.output.dense')), p + 'attention.output.LayerNorm')
        u = self.ra(F.gelu(self._lin(a1, p + 'intermediate.dense')))
        return self._ln(self.ra(a1 + self._lin(u, p + 'output.dense')), p + 'output.LayerNorm')

    def forward(self, ids, layers=None):
        """token ids [n] (special tokens in place) -> last_hidden_state [n, hidden]"""
        x = self.embed(ids)
        for i in range(self.cfg['layers'] if layers is None else layers):
            x = self.layer(x, i)
        return x

    def pooled(self, ids, mode):
        h = self.forward(ids)
        return {'mean': h.mean(dim=0), 'cls': h[0], 'max': h.max(dim=0).values}[mode]
