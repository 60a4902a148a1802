"""GPU checks of the text-encoder path against tests/text_encoder_oracle.py (itself pinned to ``transformers`` by
tests/test_text_encoder_cpu.py): the two new kernels on their own, the pass stage by stage and end to end for the BERT and the RoBERTa
configuration in fp32 and bf16 with both attention kernels, pooling, the hand-over to the resident corpus, chunking, the isolation of
sentences and the refusals.

Every comparison uses the project's rule e_dev <= 4 e_ref + 4 eps(dtype) max|oracle| (``within``, which prints the figures): e_ref is the
error of the oracle run in the device dtype (fp32, or fp32 with the tables, matrices and stored activations rounded to bf16) against
the fp64 oracle.  Shapes are the smallest that reach every path: widths below, off and on a wave's pass of the embedding kernel; sentence
lengths around the 16-row tiles and the 32-key steps of the sentence kernel, in both of its covers (32 and 64 tokens); a sentence count
that is no multiple of the four pairs of a workgroup."""
import copy
import functools

import numpy as np
import pytest
import torch

from tests import text_encoder_oracle as TO
from tests.test_pca_cpu import corpus_of

pytestmark = pytest.mark.gpu
DEV = 'cuda'
EPS = TO.EPS
TD = {'fp32': torch.float32, 'bf16': torch.bfloat16}
SIZES = {'tiny': (TO.TINY, [1, 2, 15, 16, 17, 31, 32, 33, 38], [4, 5]), 'real': (TO.REAL, [1, 7, 16, 33, 64, 20], [3, 3])}


# ---- mts_text_embed -------------------------------------------------------------------------------------------------------------------
def _embed_case(dtype, H, n=257, V=61, P=19, seed=0):
    g = torch.Generator().manual_seed(seed + H)
    rd = lambda *s: torch.randn(*s, generator=g).to(TD[dtype])          # the tables hold values of the dtype: both sides see the same numbers
    word, position, type_row = rd(V, H), rd(P, H), rd(H)
    gamma, beta = 1 + 0.1 * torch.randn(H, generator=g), 0.1 * torch.randn(H, generator=g)
    ids, pos = torch.randint(0, V, (n,), generator=g, dtype=torch.int32), torch.randint(0, P, (n,), generator=g, dtype=torch.int32)
    ids[0], ids[1], pos[0], pos[1] = V - 1, 0, P - 1, 0                  # the last and the first row of both tables
    return word, position, type_row, gamma, beta, ids, pos


def _embed_want(word, position, type_row, gamma, beta, ids, pos, ct, eps):
    x = (word.to(ct)[ids.long()] + position.to(ct)[pos.long()]) + type_row.to(ct)
    return torch.nn.functional.layer_norm(x, (x.shape[1],), gamma.to(ct), beta.to(ct), eps)


@pytest.mark.parametrize('dtype,H', [(d, h) for d in ('fp32', 'bf16') for h in (64, 200 if d == 'fp32' else 208, 384, 768, 1024)])
def test_text_embed_against_the_oracle(dtype, H):
    from multimodaltopicsegmentation_amd import ops
    word, position, type_row, gamma, beta, ids, pos = _embed_case(dtype, H)
    eps = 1e-12
    want = _embed_want(word, position, type_row, gamma, beta, ids, pos, torch.float64, eps)
    ref = _embed_want(word, position, type_row, gamma, beta, ids, pos, torch.float32, eps).to(TD[dtype])
    dev = [t.to(DEV) for t in (word, position, type_row, gamma, beta)]
    pad = 16
    for n in (1, 63, 64, 65, 257):
        out = torch.full((n, H + pad), 7.0, dtype=TD[dtype], device=DEV)
        ops.text_embed(ids[:n].to(DEV), pos[:n].to(DEV), *dev, eps, out)
        assert bool((out[:, H:] == 7.0).all()), f'columns behind H were written (n={n})'
        TO.within(out[:, :H].cpu(), want[:n], ref[:n], EPS[dtype], f'text_embed {dtype} H={H} n={n}')
        if n == 257:
            again = torch.full_like(out, 7.0)
            ops.text_embed(ids[:n].to(DEV), pos[:n].to(DEV), *dev, eps, again)
            assert torch.equal(out, again)
            tight = torch.empty((n, H), dtype=TD[dtype], device=DEV)
            ops.text_embed(ids[:n].to(DEV), pos[:n].to(DEV), *dev, eps, tight)
            assert torch.equal(tight, out[:, :H])


# the widths above reach fp32 NV = 1 .. 4 and bf16 NV = 1, 2; these reach every other instantiation of the kernel (16-byte chunks per lane x
# with / without bounds checks): fp32 256, 512 (full 1, 2), 600, 776 (3, 4 with checks), 1536, 2048 (8); bf16 512 (full 1), 1032, 1536 (3),
# 1544, 2048 (4), 2056, 4096 (8)
@pytest.mark.parametrize('dtype,H', [('fp32', h) for h in (256, 512, 600, 776, 1536, 2048)] + [('bf16', h) for h in (512, 1032, 1536, 1544, 2048, 2056, 4096)])
def test_text_embed_every_other_instantiation(dtype, H):
    from multimodaltopicsegmentation_amd import ops
    word, position, type_row, gamma, beta, ids, pos = _embed_case(dtype, H, n=66, V=9, P=5)
    want = _embed_want(word, position, type_row, gamma, beta, ids, pos, torch.float64, 1e-5)
    ref = _embed_want(word, position, type_row, gamma, beta, ids, pos, torch.float32, 1e-5).to(TD[dtype])
    out = torch.full((66, H + 8), 7.0, dtype=TD[dtype], device=DEV)
    ops.text_embed(ids.to(DEV), pos.to(DEV), *[t.to(DEV) for t in (word, position, type_row, gamma, beta)], 1e-5, out)
    assert bool((out[:, H:] == 7.0).all())
    TO.within(out[:, :H].cpu(), want, ref, EPS[dtype], f'text_embed {dtype} H={H}')


@pytest.mark.parametrize('dtype,H', [('fp32', 200), ('bf16', 208), ('fp32', 768), ('bf16', 768)])
def test_text_embed_constant_row_gives_beta_exactly(dtype, H):
    """a row whose sum is the constant 1 (0.5 + 0.25 + 0.25: the row sum H and the mean 1 are exact) has variance 0: the output is beta,
    rounded once to the dtype, whatever eps"""
    from multimodaltopicsegmentation_amd import ops
    word, position, _, gamma, beta, ids, pos = _embed_case(dtype, H, n=5)
    word[3], position[2] = 0.5, 0.25
    type_row = torch.full((H,), 0.25, dtype=TD[dtype])
    ids[2], pos[2] = 3, 2
    out = torch.empty((5, H), dtype=TD[dtype], device=DEV)
    ops.text_embed(ids.to(DEV), pos.to(DEV), word.to(DEV), position.to(DEV), type_row.to(DEV), gamma.to(DEV), beta.to(DEV), 1e-12, out)
    assert torch.equal(out[2].cpu(), beta.to(TD[dtype])) and bool(torch.isfinite(out).all())


# ---- mts_sent_attn_fwd ----------------------------------------------------------------------------------------------------------------
COVER = {32: [1, 2, 15, 16, 17, 31, 32], 64: [1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 5]}       # 7 and 11 sentences: no multiples of 4
CANARY = 7.0


def _packed(lengths, gaps=(3, 0, 2, 0, 0, 1, 0, 0, 4, 0, 0), tail=5):
    """rows of packed sentences with canary rows before, between and after -> (row0, total rows)"""
    row0, r = [], 0
    for n, gap in zip(lengths, gaps):
        r += gap
        row0.append(r)
        r += n
    return row0, r + tail


def _qkv(rows, D, heads, seed=0):
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(rows, 3 * D, generator=g)
    qkv[:, :D] *= 1.5 * (D // heads) ** -0.5                            # q already scaled: logits of order 1.5
    return qkv.to(torch.bfloat16)


def _listed(row0, lengths):
    return torch.cat([torch.arange(r, r + n) for r, n in zip(row0, lengths)])


@pytest.mark.parametrize('cover', (32, 64))
@pytest.mark.parametrize('heads', (2, 12))
@pytest.mark.parametrize('hd', (32, 64, 96, 128))
def test_sent_attn_against_the_oracle_and_the_full_kernel(hd, heads, cover):
    from multimodaltopicsegmentation_amd import ops
    lengths, D = COVER[cover], hd * heads
    row0, rows = _packed(lengths)
    qkv = _qkv(rows, D, heads, seed=hd + heads)
    want = TO.attention(qkv, lengths, row0, heads)
    ref = TO.attention(qkv, lengths, row0, heads, torch.float32).to(torch.bfloat16)
    keep = _listed(row0, lengths)
    other = torch.ones(rows, dtype=torch.bool)
    other[keep] = False
    i32 = lambda a: torch.tensor(a, dtype=torch.int32, device=DEV)
    ctx = torch.full((rows, D), CANARY, dtype=torch.bfloat16, device=DEV)
    ops.sent_attn_fwd(qkv.to(DEV), i32(row0), i32(lengths), cover, D, heads, ctx)
    assert bool((ctx[other.to(DEV)] == CANARY).all()), 'a row outside the listed sentences was written'
    TO.within(ctx[keep.to(DEV)].cpu(), want[keep], ref[keep], EPS['bf16'], f'sent_attn hd={hd} heads={heads} cover={cover}')
    again = torch.full_like(ctx, CANARY)
    ops.sent_attn_fwd(qkv.to(DEV), i32(row0), i32(lengths), cover, D, heads, again)
    assert torch.equal(ctx, again)
    full = torch.full_like(ctx, CANARY)
    lse = torch.empty((rows, heads), dtype=torch.float32, device=DEV)
    ops.full_attn_fwd(qkv.to(DEV), i32(lengths), len(lengths), cover, D, heads, full, lse, row0=i32(row0))
    TO.within(full[keep.to(DEV)].cpu(), want[keep], ref[keep], EPS['bf16'], f'full_attn hd={hd} heads={heads} cover={cover}')


def test_sent_attn_saturated_rows_are_one_hot_and_finite():
    """q_i = 12.5 e_pi(i), k_j = 16 e_j: the logit is 200 at j = pi(i) and 0 elsewhere, exp(-200) is 0 in fp32, so ctx_i is v_pi(i) exactly;
    a second head holds the negated q (logits -200 at one key, 0 elsewhere: the mean of the other keys, finite)"""
    from multimodaltopicsegmentation_amd import ops
    lengths, hd, heads = [64, 17, 1, 40, 33], 64, 2
    D = hd * heads
    row0, rows = _packed(lengths)
    g = torch.Generator().manual_seed(4)
    qkv = torch.zeros(rows, 3 * D)
    qkv[:, 2 * D:] = torch.randn(rows, D, generator=g)
    pi = lambda i, n: (7 * i + 3) % n
    for r, n in zip(row0, lengths):
        for i in range(n):
            qkv[r + i, pi(i, n)] = 12.5
            qkv[r + i, hd + pi(i, n)] = -12.5
            qkv[r + i, D + i] = qkv[r + i, D + hd + i] = 16.0
    qkv = qkv.to(torch.bfloat16)
    i32 = lambda a: torch.tensor(a, dtype=torch.int32, device=DEV)
    ctx = torch.full((rows, D), CANARY, dtype=torch.bfloat16, device=DEV)
    ops.sent_attn_fwd(qkv.to(DEV), i32(row0), i32(lengths), 64, D, heads, ctx)
    ctx = ctx.cpu()
    assert bool(torch.isfinite(ctx).all())
    for r, n in zip(row0, lengths):
        for i in range(n):
            assert torch.equal(ctx[r + i, :hd], qkv[r + pi(i, n), 2 * D:2 * D + hd]), (n, i)
    keep = _listed(row0, lengths)
    want = TO.attention(qkv, lengths, row0, heads)
    TO.within(ctx[keep], want[keep], TO.attention(qkv, lengths, row0, heads, torch.float32).to(torch.bfloat16)[keep], EPS['bf16'], 'saturated')


def test_sent_attn_refusals_leave_ctx_untouched():
    from multimodaltopicsegmentation_amd import ops
    i32 = lambda a: torch.tensor(a, dtype=torch.int32, device=DEV)
    for dtype, D, heads, max_len, word in ((torch.float32, 64, 2, 8, 'bf16 only'), (torch.bfloat16, 80, 2, 8, 'head dim 40'),
                                           (torch.bfloat16, 64, 2, 65, 'max_len=65'), (torch.bfloat16, 320, 2, 8, 'head dim 160')):
        qkv = torch.zeros((8, 3 * D), dtype=dtype, device=DEV)
        ctx = torch.full((8, D), CANARY, dtype=dtype, device=DEV)
        with pytest.raises(NotImplementedError, match=word):
            ops.sent_attn_fwd(qkv, i32([0]), i32([8]), max_len, D, heads, ctx)
        assert bool((ctx == CANARY).all())


# ---- the pass -------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _sd(size):
    return TO.random_state_dict(SIZES[size][0], seed=11)


@functools.lru_cache(maxsize=None)
def _sents(size):
    cfg, lengths, _ = SIZES[size]
    return tuple(TO.sentences(lengths, cfg['vocab'], seed=3))


@functools.lru_cache(maxsize=None)
def _oracle_states(size, family, mode, layers=None):
    """the oracle's token states of the size's sentences, computed once per configuration and shared -> [tokens, H]"""
    O = TO.Oracle(_sd(size), SIZES[size][0], mode, offset=TO.OFFSET[family])
    with torch.no_grad():
        return torch.cat([O.forward(s, layers=layers) for s in _sents(size)])


def _pool(states, size, mode):
    parts = torch.split(states, SIZES[size][1])
    return torch.stack([{'mean': p.mean(dim=0), 'cls': p[0], 'max': p.max(dim=0).values}[mode] for p in parts])


def _weights(size, family, dtype):
    from multimodaltopicsegmentation_amd import TextEncoderWeights
    return TextEncoderWeights.from_state_dict(_sd(size), TO.config_dict(SIZES[size][0], family), device=DEV, dtype=dtype)


def _text(size, sents=None):
    from multimodaltopicsegmentation_amd import ResidentText
    docs, it = [], iter(_sents(size) if sents is None else sents)
    for n in SIZES[size][2]:
        docs.append([next(it).tolist() for _ in range(n)])
    return ResidentText(docs, DEV)


def _kernels(dtype):
    return ('full', 'sentence') if dtype == 'bf16' else ('full',)


@pytest.mark.parametrize('size', ('tiny', 'real'))
@pytest.mark.parametrize('dtype', ('fp32', 'bf16'))
@pytest.mark.parametrize('family', ('bert', 'roberta'))
def test_stage_by_stage_and_end_to_end(family, dtype, size):
    from multimodaltopicsegmentation_amd import ops
    w, text, eps = _weights(size, family, dtype), _text(size), EPS[dtype]
    assert w.position_offset == TO.OFFSET[family]
    # the embedding stage on its own
    emb = torch.empty((text.total_tokens, w.hidden_size), dtype=TD[dtype], device=DEV)
    ops.text_embed(text.ids, text.positions + w.position_offset, w.word, w.position, w.type_row, w.emb_gamma, w.emb_beta, w.eps, emb)
    TO.within(emb.cpu(), _oracle_states(size, family, 'fp64', 0), _oracle_states(size, family, dtype, 0), eps, f'embeddings {family} {dtype} {size}')
    for attn in _kernels(dtype):
        what = f'{family} {dtype} {size} attn={attn}'
        # one layer, then all
        w1 = copy.copy(w)
        w1.layers, w1.num_layers = w.layers[:1], 1
        one = text.token_states(w1, out_dtype=TD[dtype], attn=attn)
        TO.within(one.frames.cpu(), _oracle_states(size, family, 'fp64', 1), _oracle_states(size, family, dtype, 1), eps, f'layer 0 {what}')
        want, ref = _oracle_states(size, family, 'fp64'), _oracle_states(size, family, dtype)
        frames = text.token_states(w, attn=attn)
        assert frames.frames.dtype == torch.float32 and frames.frames.shape == (text.total_tokens, w.hidden_size)
        assert frames.frame_counts.tolist() == SIZES[size][1] and frames.sentences.tolist() == SIZES[size][2]
        TO.within(frames.frames.cpu(), want, ref, eps, f'token_states {what}')
        for mode in ('mean', 'cls', 'max'):
            got = text.encode(w, pooling=mode, attn=attn)
            assert got.shape == (text.total_sentences, w.hidden_size) and got.dtype == torch.float32
            TO.within(got.cpu(), _pool(want, size, mode), _pool(ref.double(), size, mode), eps, f"encode('{mode}') {what}")
        TO.within(frames.pool('mean').cpu(), _pool(want, size, 'mean'), _pool(ref.double(), size, 'mean'), eps, f"pool('mean') {what}")
        # into a corpus
        rows = text.sentences.tolist()
        other = np.ascontiguousarray(np.random.default_rng(5).integers(-8, 9, size=(sum(rows), 6)).astype(np.float32))
        fused = corpus_of(other, rows, DEV).with_frames(frames, 'mean', field='embeddings2')
        assert torch.equal(fused.corpus2, frames.pool('mean', out_dtype=fused.corpus2.dtype))
        TO.within(fused.corpus2.cpu(), _pool(want, size, 'mean'), _pool(ref.double(), size, 'mean'), eps, f'with_frames {what}')
        # several chunks: a budget of some forty tokens
        e = 2 if dtype == 'bf16' else 4
        small = 40 * (e * (9 * w.hidden_size + w.intermediate_size) + 4 * w.hidden_size + 4 * (w.num_heads + 2) + 16)
        assert len(text._chunks('token_states', w, torch.float32, small, attn)) >= 3
        split = text.token_states(w, attn=attn, workspace_bytes=small)
        between = float((split.frames - frames.frames).abs().max())
        bound = 4 * float((ref.double() - want).abs().max()) + 4 * eps * float(want.abs().max())
        print(f'chunked against one chunk {what}: {between:.3e} (bound {bound:.3e})')
        assert between <= bound
        TO.within(split.frames.cpu(), want, ref, eps, f'chunked token_states {what}')
        pooled = text.encode(w, attn=attn, workspace_bytes=small)
        TO.within(pooled.cpu(), _pool(want, size, 'mean'), _pool(ref.double(), size, 'mean'), eps, f'chunked encode {what}')


def test_auto_dispatch_follows_the_cover():
    """'auto' takes the sentence kernel for a chunk it covers with bf16 weights, the full kernel for a chunk with a longer sentence and for
    fp32; the mixed pass gives the oracle's states"""
    from multimodaltopicsegmentation_amd import ResidentText
    cfg = TO.REAL
    g = torch.Generator().manual_seed(8)
    sents = [torch.randint(0, cfg['vocab'], (n,), generator=g) for n in (64, 3, 65, 70, 12)]
    text = ResidentText([[s.tolist() for s in sents]], DEV)
    w = _weights('real', 'roberta', 'bf16')
    assert [k for _, _, k in text._chunks('encode', w, torch.float32, None, 'auto')] == ['full']
    per = 2 * (9 * w.hidden_size + w.intermediate_size) + 4 * w.hidden_size + 4 * (w.num_heads + 2) + 16
    assert [(a, b, k) for a, b, k in text._chunks('encode', w, torch.float32, 70 * per, 'auto')] == [(0, 2, 'sentence'), (2, 3, 'full'), (3, 4, 'full'), (4, 5, 'sentence')]
    assert [k for _, _, k in text._chunks('encode', _weights('real', 'roberta', 'fp32'), torch.float32, 70 * 2 * per, 'auto')] == ['full'] * 4
    with pytest.raises(NotImplementedError, match="attn='sentence'"):
        text.token_states(w, attn='sentence')
    O, R = (TO.Oracle(_sd('real'), cfg, m, offset=2) for m in ('fp64', 'bf16'))
    with torch.no_grad():
        want, ref = torch.cat([O.forward(s) for s in sents]), torch.cat([R.forward(s) for s in sents])
    TO.within(text.token_states(w, workspace_bytes=70 * per).frames.cpu(), want, ref, EPS['bf16'], 'auto, mixed chunks')


@pytest.mark.parametrize('attn', ('full', 'sentence'))
def test_sentences_are_isolated(attn):
    """changing the tokens of one sentence leaves every other sentence's rows bit for bit"""
    w = _weights('tiny', 'roberta', 'bf16')
    sents = list(_sents('tiny'))
    before = _text('tiny').token_states(w, attn=attn).frames
    k = 4
    changed = list(sents)
    changed[k] = (sents[k] + 1) % TO.TINY['vocab']
    after = _text('tiny', changed).token_states(w, attn=attn).frames
    start = np.concatenate([[0], np.cumsum(SIZES['tiny'][1])])
    a, b = int(start[k]), int(start[k + 1])
    assert torch.equal(before[:a], after[:a]) and torch.equal(before[b:], after[b:])
    assert not torch.equal(before[a:b], after[a:b])


def test_refusals_come_before_any_launch():
    from multimodaltopicsegmentation_amd import ResidentText
    w32, w16 = _weights('tiny', 'bert', 'fp32'), _weights('tiny', 'bert', 'bf16')
    with pytest.raises(ValueError, match='token id 97'):
        ResidentText([[[3, 97]]], DEV).encode(w32)
    with pytest.raises(ValueError, match='longest sentence has 41 tokens'):
        ResidentText([[[5] * 41]], DEV).token_states(w16)
    with pytest.raises(ValueError, match='longest sentence has 39 tokens'):
        ResidentText([[[5] * 39]], DEV).token_states(_weights('tiny', 'roberta', 'bf16'))
    with pytest.raises(NotImplementedError, match="attn='sentence' needs bf16"):
        _text('tiny').encode(w32, attn='sentence')
    with pytest.raises(ValueError, match='weights must be a TextEncoderWeights'):
        _text('tiny').encode(object())
    from multimodaltopicsegmentation_amd import TextEncoderWeights
    host = TextEncoderWeights.from_state_dict(_sd('tiny'), TO.config_dict(TO.TINY, 'bert'), device='cpu', dtype='bf16')
    with pytest.raises(ValueError, match='the weights live on cpu'):
        _text('tiny').encode(host)
