"""CPU checks of the text-encoder path: the tests' oracle against ``transformers`` (random weights, built offline from a config), mean
pooling against sentence-transformers' definition, ``TextEncoderWeights.from_state_dict`` and ``ResidentText`` on the host,
``tokenize_documents`` with a WordPiece tokenizer built in line, and the ABI of the two new entry points."""
import os
import re

import numpy as np
import pytest
import torch

from tests import text_encoder_oracle as TO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRY_POINTS = ('mts_text_embed', 'mts_sent_attn_fwd')
FAMILIES = ('bert', 'roberta', 'xlm-roberta')
LENGTHS = (1, 2, 7, 38)


def _hf_model(family, cfg=TO.TINY):
    """a transformers model of the family at the oracle's size, holding ``random_state_dict``'s weights -> (model in fp64, pad id)"""
    tr = pytest.importorskip('transformers')
    kw = dict(vocab_size=cfg['vocab'], hidden_size=cfg['hidden'], num_hidden_layers=cfg['layers'], num_attention_heads=cfg['heads'],
              intermediate_size=cfg['intermediate'], max_position_embeddings=cfg['positions'], hidden_dropout_prob=0.0,
              attention_probs_dropout_prob=0.0, layer_norm_eps=cfg['eps'], hidden_act='gelu', type_vocab_size=2)
    if family == 'bert':
        hc, cls = tr.BertConfig(pad_token_id=0, **kw), tr.BertModel
    elif family == 'roberta':
        hc, cls = tr.RobertaConfig(pad_token_id=1, bos_token_id=0, eos_token_id=2, **kw), tr.RobertaModel
    else:
        hc, cls = tr.XLMRobertaConfig(pad_token_id=1, bos_token_id=0, eos_token_id=2, **kw), tr.XLMRobertaModel
    model = cls(hc).eval()
    res = model.load_state_dict(TO.random_state_dict(cfg, seed=3), strict=False)
    assert not res.unexpected_keys and all(k.startswith('pooler.') or k.endswith(('position_ids', 'token_type_ids')) for k in res.missing_keys), res
    return model.double(), hc


def _ids(cfg=TO.TINY, seed=7):
    """sentences of LENGTHS; ids from 3 up, so that no token is a pad id (RoBERTa derives the positions from it)"""
    g = torch.Generator().manual_seed(seed)
    return [torch.randint(3, cfg['vocab'], (n,), generator=g) for n in LENGTHS]


def _padded(sents, pad):
    n = max(len(s) for s in sents)
    ids = torch.full((len(sents), n), pad, dtype=torch.long)
    mask = torch.zeros((len(sents), n), dtype=torch.long)
    for i, s in enumerate(sents):
        ids[i, :len(s)], mask[i, :len(s)] = s, 1
    return ids, mask


@pytest.mark.parametrize('family', FAMILIES)
def test_oracle_equals_transformers(family):
    model, hc = _hf_model(family)
    O = TO.Oracle(model.state_dict(), TO.TINY, 'fp64', offset=TO.OFFSET[family])
    sents = _ids()
    ids, mask = _padded(sents, hc.pad_token_id)
    with torch.no_grad():
        batch = model(input_ids=ids, attention_mask=mask).last_hidden_state
        for i, s in enumerate(sents):
            alone = model(input_ids=s[None]).last_hidden_state[0]
            got = O.forward(s)
            assert got.shape == alone.shape == (len(s), TO.TINY['hidden'])
            e_alone, e_batch = float((got - alone).abs().max()), float((got - batch[i, :len(s)]).abs().max())
            print(f'{family} length {len(s)}: |oracle - alone| {e_alone:.3e}, |oracle - in padded batch| {e_batch:.3e}')
            # the position offset (2 for the RoBERTa family, 0 for BERT) is pinned here: another offset reads other rows of the table
            assert e_alone <= 1e-12 and e_batch <= 1e-12
        # the embedding stage on its own: word[ids] + position[arange + offset] + type[0] under the LayerNorm
        for s in sents:
            assert float((O.embed(s) - model.embeddings(input_ids=s[None])[0]).abs().max()) <= 1e-13


@pytest.mark.parametrize('family', ('bert', 'roberta'))
def test_mean_pooling_is_sentence_transformers_definition(family):
    model, hc = _hf_model(family)
    O = TO.Oracle(model.state_dict(), TO.TINY, 'fp64', offset=TO.OFFSET[family])
    sents = _ids(seed=9)
    ids, mask = _padded(sents, hc.pad_token_id)
    with torch.no_grad():
        h = model(input_ids=ids, attention_mask=mask).last_hidden_state
    m = mask[:, :, None].to(h.dtype)
    want = (h * m).sum(dim=1) / torch.clamp(m.sum(dim=1), min=1e-9)         # sentence_transformers.models.Pooling, mode 'mean'
    got = torch.stack([O.pooled(s, 'mean') for s in sents])
    assert float((got - want).abs().max()) <= 1e-12
    assert float((torch.stack([O.pooled(s, 'cls') for s in sents]) - h[:, 0]).abs().max()) <= 1e-12


def test_oracle_modes_differ_only_by_rounding():
    sd = TO.random_state_dict(TO.TINY, seed=1)
    s = _ids()[3]
    want = TO.Oracle(sd, TO.TINY, 'fp64', offset=2).forward(s)
    e32 = float((TO.Oracle(sd, TO.TINY, 'fp32', offset=2).forward(s).double() - want).abs().max())
    e16 = float((TO.Oracle(sd, TO.TINY, 'bf16', offset=2).forward(s).double() - want).abs().max())
    assert 0 < e32 < 1e-4 < e16 < 0.2, (e32, e16)


# ---- TextEncoderWeights ---------------------------------------------------------------------------------------------------------------
def _weights(sd, family='roberta', **kw):
    from multimodaltopicsegmentation_amd.text import TextEncoderWeights
    return TextEncoderWeights.from_state_dict(sd, kw.pop('config', TO.config_dict(TO.TINY, family)), **kw)


def test_from_state_dict_layout_prefixes_and_round_trip():
    sd = TO.random_state_dict(TO.TINY, seed=2)
    w = _weights(sd, dtype='fp32')
    assert (w.vocab_size, w.hidden_size, w.num_layers, w.num_heads, w.intermediate_size, w.max_position_embeddings) == (97, 64, 2, 2, 128, 40)
    assert w.position_offset == 2 and w.eps == 1e-12 and w.dtype == torch.float32
    assert _weights(sd, 'bert').position_offset == 0 and _weights(sd, 'xlm-roberta').position_offset == 2
    assert _weights(sd, 'bert', position_offset=5).position_offset == 5             # the explicit argument wins
    assert _weights(sd, config={'num_attention_heads': 1, 'layer_norm_eps': 1e-5}).position_offset == 0     # no model_type: BERT's offset
    assert torch.equal(w.type_row, sd['embeddings.token_type_embeddings.weight'][0]) and w.type_row.shape == (64,)
    assert torch.equal(w.word, sd['embeddings.word_embeddings.weight']) and torch.equal(w.position, sd['embeddings.position_embeddings.weight'])
    for i, p in enumerate(w.layers):
        a = f'encoder.layer.{i}.attention.self.'
        assert p['qkv_w'].shape == (192, 64) and p['qkv_b'].shape == (192,)
        for j, n in enumerate(('query', 'key', 'value')):
            assert torch.equal(p['qkv_w'][64 * j:64 * (j + 1)], sd[a + n + '.weight']) and torch.equal(p['qkv_b'][64 * j:64 * (j + 1)], sd[a + n + '.bias'])
        assert torch.equal(p['ff1_w'], sd[f'encoder.layer.{i}.intermediate.dense.weight']) and torch.equal(p['ln2_b'], sd[f'encoder.layer.{i}.output.LayerNorm.bias'])
    w16 = _weights(sd, dtype='bf16')
    assert w16.word.dtype == w16.layers[0]['qkv_w'].dtype == torch.bfloat16 and w16.layers[0]['qkv_b'].dtype == w16.emb_gamma.dtype == torch.float32
    assert torch.equal(w16.word, sd['embeddings.word_embeddings.weight'].to(torch.bfloat16))
    # prefixes are stripped, what is no part of the encoder is ignored
    extra = {'pooler.dense.weight': torch.zeros(64, 64), 'pooler.dense.bias': torch.zeros(64), 'embeddings.position_ids': torch.arange(40)[None],
             'embeddings.token_type_ids': torch.zeros(1, 40, dtype=torch.long)}
    heads = {'cls.predictions.bias': torch.zeros(97), 'lm_head.dense.weight': torch.zeros(64, 64), 'lm_head.bias': torch.zeros(97)}
    for prefix in ('bert.', 'roberta.', '0.auto_model.', '0.auto_model.roberta.'):
        other = _weights({**{prefix + k: v for k, v in {**sd, **extra}.items()}, **heads}, dtype='fp32')
        assert set(other.state_dict()) == set(sd)
        assert all(torch.equal(a[k], b[k]) for a, b in zip(w.layers, other.layers) for k in a) and torch.equal(other.word, w.word)
    # the round trip
    again = type(w).from_state_dict(w.state_dict(), w.config(), dtype='fp32')
    assert again.config() == w.config() == {'num_attention_heads': 2, 'layer_norm_eps': 1e-12, 'position_offset': 2}
    assert set(again.state_dict()) == set(sd) and all(torch.equal(again.state_dict()[k], sd[k]) for k in sd)
    assert all(torch.equal(a[k], b[k]) for a, b in zip(w.layers, again.layers) for k in a) and torch.equal(again.type_row, w.type_row)
    assert w.sent_attn_covers(64) is False and w16.sent_attn_covers(64) and not w16.sent_attn_covers(65)


def test_from_state_dict_refusals_name_their_cause():
    sd = TO.random_state_dict(TO.TINY, seed=2)
    base = TO.config_dict(TO.TINY, 'bert')
    for change, word in (({'position_embedding_type': 'relative_key'}, 'relative_key'), ({'hidden_act': 'relu'}, "'relu'"),
                         ({'is_decoder': True}, 'decoder'), ({'add_cross_attention': True}, 'cross-attention'), ({'embedding_size': 32}, 'embedding_size=32')):
        with pytest.raises(NotImplementedError, match=re.escape(word)):
            _weights(sd, config={**base, **change})
    with pytest.raises(NotImplementedError, match='distance_embedding|relative'):
        _weights({**sd, 'encoder.layer.0.attention.self.distance_embedding.weight': torch.zeros(79, 32)}, config=base)
    with pytest.raises(NotImplementedError, match='cross-attention'):
        _weights({**sd, 'encoder.layer.0.crossattention.self.query.weight': torch.zeros(64, 64)}, config=base)
    narrow = dict(sd)
    narrow['embeddings.word_embeddings.weight'] = torch.zeros(97, 32)
    with pytest.raises(NotImplementedError, match='embedding_size=32'):
        _weights(narrow, config=base)
    with pytest.raises(NotImplementedError, match='head dim 4 '):
        _weights(sd, config={**base, 'num_attention_heads': 16}, dtype='bf16')
    with pytest.raises(ValueError, match='not divisible by 3 heads'):
        _weights(sd, config={**base, 'num_attention_heads': 3})
    with pytest.raises(ValueError, match='word_embeddings'):
        _weights({k: v for k, v in sd.items() if 'word_embeddings' not in k}, config=base)
    with pytest.raises(ValueError, match='dtype'):
        _weights(sd, dtype='fp16')
    for missing in ('num_attention_heads', 'layer_norm_eps'):                        # nothing is guessed
        with pytest.raises(ValueError, match=f'must give {missing}'):
            _weights(sd, config={k: v for k, v in base.items() if k != missing})
    with pytest.raises(ValueError, match='must give num_attention_heads'):
        type(_weights(sd)).from_state_dict(sd)
    with pytest.raises(ValueError, match='position_offset=40'):
        _weights(sd, config=base, position_offset=40)


# ---- ResidentText, tokenize_documents -------------------------------------------------------------------------------------------------
def test_resident_text_tables_and_host_refusals():
    from multimodaltopicsegmentation_amd.text import ResidentText
    docs = [[[5, 6, 7], [8]], [np.array([1, 96, 3, 4, 2]), torch.tensor([9, 9])], [(0,)]]
    t = ResidentText(docs, 'cpu')
    assert (t.n_docs, t.total_sentences, t.total_tokens, t.max_id, t.max_len, len(t)) == (3, 5, 12, 96, 5, 3)
    assert t.sentences.tolist() == [2, 2, 1] and t.token_counts.tolist() == [3, 1, 5, 2, 1]
    assert t.host_tok_start.tolist() == [0, 3, 4, 9, 11, 12] and t.host_tok_start.dtype == np.int64
    assert t.host_ids.tolist() == [5, 6, 7, 8, 1, 96, 3, 4, 2, 9, 9, 0] and t.host_ids.dtype == np.int32
    assert t.host_positions.tolist() == [0, 1, 2, 0, 0, 1, 2, 3, 4, 0, 1, 0] and t.host_positions.dtype == np.int32
    assert t.ids is None and t.nbytes == 0
    for bad, word in (([], 'no documents'), ([[[1]], []], 'document 1 has no sentences'), ([[[1], []]], 'sentence 1 of document 0 is empty'),
                      ([[[1]], [[2, -3]]], 'sentence 0 of document 1 holds the negative id -3'), ([[[1.5]]], 'integers')):
        with pytest.raises(ValueError, match=word):
            ResidentText(bad, 'cpu')
    # the refusals of a pass that need no device: all come before the first launch
    w = _weights(TO.random_state_dict(TO.TINY, seed=2), dtype='fp32')
    with pytest.raises(ValueError, match='token id 97'):
        ResidentText([[[3, 97]]], 'cpu').encode(w)
    with pytest.raises(ValueError, match='longest sentence has 39 tokens'):
        ResidentText([[list(range(39))]], 'cpu').token_states(w)
    with pytest.raises(NotImplementedError, match="attn='sentence'"):
        t.encode(w, attn='sentence')
    with pytest.raises(ValueError, match='pooling'):
        t.encode(w, pooling='last')
    with pytest.raises(ValueError, match='attn is'):
        t.encode(w, attn='flash')
    with pytest.raises(RuntimeError, match='runs on the GPU'):
        t.encode(w)


def _wordpiece():
    tk = pytest.importorskip('tokenizers')
    vocab = {w: i for i, w in enumerate(['[PAD]', '[UNK]', '[CLS]', '[SEP]', 'the', 'news', 'to', '##day', 'is', 'good', 'weather', '##s', 'rain'])}
    tok = tk.Tokenizer(tk.models.WordPiece(vocab, unk_token='[UNK]'))
    tok.normalizer = tk.normalizers.Lowercase()
    tok.pre_tokenizer = tk.pre_tokenizers.Whitespace()
    tok.post_processor = tk.processors.TemplateProcessing(single='[CLS] $A [SEP]', special_tokens=[('[CLS]', 2), ('[SEP]', 3)])
    return tok


def test_tokenize_documents_wordpiece_and_truncation():
    from multimodaltopicsegmentation_amd.text import ResidentText, tokenize_documents
    tok = _wordpiece()
    docs = [['The news today is good', 'Rain'], ['the weathers today is the news today is good zebra']]
    ids = tokenize_documents(docs, tok)
    assert ids == [[[2, 4, 5, 6, 7, 8, 9, 3], [2, 12, 3]], [[2, 4, 10, 11, 6, 7, 8, 4, 5, 6, 7, 8, 9, 1, 3]]]
    assert tok.truncation is None                                   # the caller's tokenizer is handed back as it came
    cut = tokenize_documents(docs, tok, max_length=6)
    assert cut == [[[2, 4, 5, 6, 7, 3], [2, 12, 3]], [[2, 4, 10, 11, 6, 3]]]      # six ids INCLUDING [CLS] and [SEP], which stay
    tok.enable_truncation(max_length=4)
    assert tokenize_documents(docs, tok, max_length=6) == cut and tok.truncation['max_length'] == 4
    t = ResidentText(cut, 'cpu')
    assert t.max_len == 6 and t.token_counts.tolist() == [6, 3, 6]
    with pytest.raises(ValueError, match='max_length'):
        tokenize_documents(docs, tok, max_length=0)
    # a Hugging Face tokenizer callable gives the same ids
    tr = pytest.importorskip('transformers')
    tok.no_truncation()
    fast = tr.PreTrainedTokenizerFast(tokenizer_object=tok, unk_token='[UNK]', pad_token='[PAD]', cls_token='[CLS]', sep_token='[SEP]')
    assert tokenize_documents(docs, fast, max_length=6) == cut and tokenize_documents(docs, fast) == ids


def test_new_entry_points_are_declared_bound_and_documented():
    from multimodaltopicsegmentation_amd import _lib as L
    from tests.test_abi import _declared
    decl = _declared()
    doc = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    for name in NEW_ENTRY_POINTS:
        assert name in decl, f'{name} is not declared in include/mts.h'
        assert hasattr(L.lib, name) and len(L.SIGNATURES[name][1]) == decl[name], name
        assert re.search(r'`' + name + r'`', doc), f'{name} is missing from INTEGRATION.md'
    # argument validation happens before any device work: safe without a GPU
    p = 4096                                                        # stands for a device address: never dereferenced by a refused call
    embed = lambda dtype=0, n=1, H=64, ids=p, ldo=64, eps=1e-5, out=p: L.lib.mts_text_embed(None, dtype, n, H, ids, p, p, 10, p, 10, p, p, p, eps, out, ldo)
    assert embed(n=0) == 1 and embed(ids=None) == 1 and embed(dtype=7) == 1 and embed(eps=-1.0) == 1
    assert embed(H=66, ldo=68) == 2 and embed(dtype=1, H=68, ldo=72) == 2 and embed(H=2052, ldo=2052) == 2 and embed(dtype=1, H=4104, ldo=4104) == 2
    assert embed(ldo=60) == 1 and embed(dtype=1, ldo=68) == 1 and embed(out=p + 8) == 1
    attn = lambda dtype=1, n=1, D=64, heads=2, qkv=p, max_len=10: L.lib.mts_sent_attn_fwd(None, dtype, n, D, heads, qkv, p, p, max_len, p)
    assert attn(n=0) == 1 and attn(qkv=None) == 1 and attn(dtype=7) == 1 and attn(heads=3) == 1 and attn(max_len=0) == 1
    assert attn(dtype=0) == 2 and attn(D=80) == 2 and attn(D=320) == 2 and attn(max_len=65) == 2
    with pytest.raises(NotImplementedError, match='max_len=65'):
        L.check(attn(max_len=65))
