"""BERT / RoBERTa sentence embeddings from resident token ids: the reference's text encoder on the device.

Every run script of the reference feeds a folder of RoBERTa sentence embeddings next to the audio one, and its ``--online_encoding`` path
is ``SentenceTransformer(name).encode(sentence)`` per sentence on the host (EncoderDataset.py:238-250; default ``--encoder
stsb-bert-base``).  Here the token ids of a whole corpus are uploaded ONCE (``ResidentText``) and ``text.token_states(weights)`` makes
``BertModel / RobertaModel / XLMRobertaModel(...).last_hidden_state`` of every sentence in HBM, a chunk of sentences at a time, as a
``frames.ResidentFrames`` whose ``pool('mean')`` is sentence-transformers' mean pooling over the attended tokens and which
``ResidentCorpus.with_frames`` takes unchanged.  ``text.encode(weights, pooling)`` pools chunk by chunk without keeping the token states.
Inference only.  Tokenisation stays on the host and is the user's tokenizer (``tokenize_documents`` is a thin helper around it); L2
normalisation (sentence-transformers' ``Normalize`` module) is not applied.

The pass of a chunk: sentences are packed one after another ([tokens, H] rows, no padding), ``ops.text_embed`` (csrc/text_encoder.hip)
writes LayerNorm(word + position + type 0), and the post-LN layers are ``wav2vec2.encoder_layers`` -- the GEMMs with their bias / GELU /
residual epilogues, the LayerNorms and an attention kernel that keeps every sentence a sequence of its own (``lengths`` / ``row0``):
``mts_sent_attn_fwd`` (one wave per sentence and head; bf16, sentences up to 64 tokens) or ``mts_full_attn_fwd``.
"""
import numpy as np
import torch

from .frames import ResidentFrames
from .wav2vec2 import ACT_DTYPES, cfg_get

_PREFIXES = ('0.auto_model.', 'bert.', 'roberta.')
_IGNORED = ('pooler.', 'embeddings.position_ids', 'embeddings.token_type_ids', 'cls.', 'lm_head.', 'classifier.', 'qa_outputs.')
_OFFSET_FAMILY = ('roberta', 'xlm-roberta', 'xlm-roberta-xl', 'camembert')      # positions start at pad_token_id + 1
SENT_ATTN_MAX_LEN = 64                       # tokens mts_sent_attn_fwd covers
POOLINGS = ('mean', 'cls', 'max')


def _strip(key):
    stripped = True
    while stripped:
        stripped = False
        for p in _PREFIXES:
            if key.startswith(p):
                key, stripped = key[len(p):], True
    return key


class TextEncoderWeights:
    """The parameters of a Hugging Face ``BertModel`` / ``RobertaModel`` / ``XLMRobertaModel`` laid out once for the kernels (use
    ``from_state_dict``).

    Host attributes: ``vocab_size``, ``max_position_embeddings``, ``hidden_size`` H, ``intermediate_size``, ``num_layers``, ``num_heads``,
    ``eps``, ``position_offset`` (the position-table row of a sentence's first token: pad_token_id + 1 for the RoBERTa family, 0 for
    BERT), ``dtype`` (torch.float32 | torch.bfloat16), ``device``.  Tensors on ``device``: in ``dtype`` ``word`` [vocab, H], ``position``
    [positions, H], ``type_row`` [H] (token type 0, the only one used), per layer ``qkv_w`` [3 H, H] (q | k | v), ``o_w``, ``ff1_w``,
    ``ff2_w``; fp32 biases and LayerNorm parameters."""

    @classmethod
    def from_state_dict(cls, sd, config=None, device='cpu', dtype='bf16', position_offset=None):
        if dtype not in ACT_DTYPES:
            raise ValueError("TextEncoderWeights: dtype must be 'bf16' or 'fp32'")
        src = {}
        for k, t in sd.items():
            if k.startswith(_IGNORED):
                continue
            k = _strip(k)
            if k.startswith(_IGNORED):
                continue
            src[k] = t.detach().to('cpu', torch.float32).contiguous()
        e = 'embeddings.'
        if e + 'word_embeddings.weight' not in src:
            raise ValueError('TextEncoderWeights: the state dict holds no embeddings.word_embeddings.weight')
        kind = cfg_get(config, 'position_embedding_type', None) or 'absolute'
        if kind != 'absolute' or any('distance_embedding' in k for k in src):
            raise NotImplementedError(f'TextEncoderWeights: position_embedding_type={kind!r} (relative position embeddings); only '
                                      "'absolute' is supported")
        if cfg_get(config, 'hidden_act', 'gelu') != 'gelu':
            raise NotImplementedError(f"TextEncoderWeights: hidden_act={cfg_get(config, 'hidden_act')!r}; only 'gelu' is supported")
        if cfg_get(config, 'is_decoder', False) or cfg_get(config, 'add_cross_attention', False) or any('crossattention' in k for k in src):
            raise NotImplementedError('TextEncoderWeights: a decoder / cross-attention configuration (is_decoder or add_cross_attention); only '
                                      'the encoder is supported')
        word = src[e + 'word_embeddings.weight']
        V, E = (int(d) for d in word.shape)
        L = 0
        while f'encoder.layer.{L}.attention.self.query.weight' in src:
            L += 1
        H = int(src['encoder.layer.0.attention.self.query.weight'].shape[1]) if L else E
        if E != H or int(cfg_get(config, 'embedding_size', E) or E) != H:
            raise NotImplementedError(f'TextEncoderWeights: embedding_size={cfg_get(config, "embedding_size", E)} differs from hidden_size={H} (a '
                                      'factorised embedding); only embedding_size == hidden_size is supported')
        self = cls.__new__(cls)
        self.dtype, self.device = ACT_DTYPES[dtype], torch.device(device)
        if self.device.type == 'cuda' and self.device.index is None:
            self.device = torch.device('cuda', torch.cuda.current_device())
        self.vocab_size, self.hidden_size, self.num_layers = V, H, L
        self.max_position_embeddings = int(src[e + 'position_embeddings.weight'].shape[0])
        for name in ('num_attention_heads', 'layer_norm_eps'):
            if cfg_get(config, name, None) is None:
                raise ValueError(f'TextEncoderWeights: the config must give {name} (the tensors cannot tell it, and a guess would give plausible '
                                 'but wrong embeddings)')
        self.num_heads = int(cfg_get(config, 'num_attention_heads'))
        if H % self.num_heads:
            raise ValueError(f'TextEncoderWeights: hidden size {H} is not divisible by {self.num_heads} heads')
        hd, vec = H // self.num_heads, 4 if self.dtype == torch.float32 else 8
        if hd % vec or hd > 512 or H % vec:
            raise NotImplementedError(f'TextEncoderWeights: head dim {hd} in {dtype}; the attention kernels take multiples of {vec} up to 512')
        self.eps = float(cfg_get(config, 'layer_norm_eps'))
        if position_offset is None:
            position_offset = cfg_get(config, 'position_offset', None)
        if position_offset is None:
            family = str(cfg_get(config, 'model_type', 'bert')).lower()
            pad = cfg_get(config, 'pad_token_id', None)
            position_offset = (1 if pad is None else int(pad)) + 1 if family in _OFFSET_FAMILY else 0
        self.position_offset = int(position_offset)
        if not 0 <= self.position_offset < self.max_position_embeddings:
            raise ValueError(f'TextEncoderWeights: position_offset={self.position_offset} outside the {self.max_position_embeddings} positions')
        self.intermediate_size = int(src['encoder.layer.0.intermediate.dense.weight'].shape[0]) if L else 0
        self._src = src

        act = lambda t: t.to(self.dtype).contiguous().to(self.device)
        f32 = lambda t: t.to(torch.float32).contiguous().to(self.device)
        self.word, self.position = act(word), act(src[e + 'position_embeddings.weight'])
        self.type_row = act(src[e + 'token_type_embeddings.weight'][0])
        self.emb_gamma, self.emb_beta = f32(src[e + 'LayerNorm.weight']), f32(src[e + 'LayerNorm.bias'])
        self.layers = []
        for i in range(L):
            p = f'encoder.layer.{i}.'
            a = p + 'attention.self.'
            self.layers.append({
                'qkv_w': act(torch.cat([src[a + f'{n}.weight'] for n in ('query', 'key', 'value')])),
                'qkv_b': f32(torch.cat([src[a + f'{n}.bias'] for n in ('query', 'key', 'value')])),
                'o_w': act(src[p + 'attention.output.dense.weight']), 'o_b': f32(src[p + 'attention.output.dense.bias']),
                'ln1_g': f32(src[p + 'attention.output.LayerNorm.weight']), 'ln1_b': f32(src[p + 'attention.output.LayerNorm.bias']),
                'ff1_w': act(src[p + 'intermediate.dense.weight']), 'ff1_b': f32(src[p + 'intermediate.dense.bias']),
                'ff2_w': act(src[p + 'output.dense.weight']), 'ff2_b': f32(src[p + 'output.dense.bias']),
                'ln2_g': f32(src[p + 'output.LayerNorm.weight']), 'ln2_b': f32(src[p + 'output.LayerNorm.bias'])})
        return self

    def state_dict(self):
        """-> the fp32 host tensors ``from_state_dict`` took, under Hugging Face's names without a prefix:
        ``from_state_dict(w.state_dict(), w.config())`` gives the same weights"""
        return dict(self._src)

    def config(self):
        """what the tensors cannot tell, as a dict ``from_state_dict`` takes"""
        return {'num_attention_heads': self.num_heads, 'layer_norm_eps': self.eps, 'position_offset': self.position_offset}

    def sent_attn_covers(self, max_len):
        """does mts_sent_attn_fwd cover a chunk of these weights whose longest sentence has ``max_len`` tokens?"""
        hd = self.hidden_size // self.num_heads
        return self.dtype == torch.bfloat16 and hd % 32 == 0 and hd <= 128 and int(max_len) <= SENT_ATTN_MAX_LEN


def tokenize_documents(docs_of_strings, tokenizer, max_length=128):
    """documents of sentence strings -> the nested id lists ``ResidentText`` takes.  ``tokenizer``: a ``tokenizers.Tokenizer`` (its
    ``encode_batch``; truncation is switched on for the call and put back) or a Hugging Face tokenizer callable.  A sentence is cut to
    ``max_length`` ids INCLUDING its special tokens, which stay in place.  Tokenisation itself is the tokenizer's and runs on the host."""
    if int(max_length) < 1:
        raise ValueError(f'tokenize_documents: max_length must be positive, not {max_length}')
    out = []
    if hasattr(tokenizer, 'encode_batch') and hasattr(tokenizer, 'enable_truncation'):
        before = tokenizer.truncation
        tokenizer.enable_truncation(max_length=int(max_length))
        try:
            for doc in docs_of_strings:
                out.append([list(e.ids) for e in tokenizer.encode_batch(list(doc))])
        finally:
            if before is None:
                tokenizer.no_truncation()
            else:
                tokenizer.enable_truncation(**before)
        return out
    for doc in docs_of_strings:
        enc = tokenizer(list(doc), truncation=True, max_length=int(max_length), add_special_tokens=True)
        out.append([list(ids) for ids in enc['input_ids']])
    return out


class ResidentText:
    """The token ids of a corpus in HBM, uploaded ONCE: ``ids`` and ``positions`` (int32 [total_tokens]: a token's id and its place in
    its sentence, from 0), ``tok_start`` (int64 [total_sentences + 1]: sentence s is tokens tok_start[s] .. tok_start[s + 1]),
    ``lengths`` (int32 [total_sentences]) and ``doc_sentences`` (int64 [n_docs]).  ``docs``: a list of documents, each a list of
    sentences, each a sequence of token ids with its special tokens already in place (what a tokenizer returns).  Host tables:
    ``sentences`` (sentences per document), ``token_counts``, ``host_ids``, ``host_positions``, ``host_tok_start``, ``n_docs``,
    ``total_sentences``, ``total_tokens``, ``max_id``, ``max_len``.
    With a CPU device only the host tables exist, as for ResidentCorpus.

    ValueError, naming the document and the sentence: no documents, a document without sentences, an empty sentence, a negative id."""

    WORKSPACE = 1 << 30                       # bytes of activations a chunk of sentences may take

    def __init__(self, docs, device):
        self.device = torch.device(device)
        if self.device.type == 'cuda' and self.device.index is None:
            self.device = torch.device('cuda', torch.cuda.current_device())
        if len(docs) == 0:
            raise ValueError('ResidentText: no documents')
        parts, counts, sentences = [], [], []
        for d, doc in enumerate(docs):
            if len(doc) == 0:
                raise ValueError(f'ResidentText: document {d} has no sentences')
            sentences.append(len(doc))
            for s, ids in enumerate(doc):
                a = np.asarray(ids.detach().cpu().numpy() if isinstance(ids, torch.Tensor) else ids).reshape(-1)
                if a.size == 0:
                    raise ValueError(f'ResidentText: sentence {s} of document {d} is empty (a tokenizer returns at least its special tokens)')
                if a.dtype.kind not in 'iu':
                    raise ValueError(f'ResidentText: sentence {s} of document {d} holds {a.dtype} values; token ids are integers')
                a = a.astype(np.int64)
                if a.min() < 0:
                    raise ValueError(f'ResidentText: sentence {s} of document {d} holds the negative id {int(a.min())}')
                parts.append(a)
                counts.append(int(a.size))
        self.n_docs = len(sentences)
        self.sentences = np.asarray(sentences, dtype=np.int64)
        self.token_counts = np.asarray(counts, dtype=np.int64)
        self.total_sentences = int(self.sentences.sum())
        start = np.zeros(self.total_sentences + 1, dtype=np.int64)
        np.cumsum(self.token_counts, out=start[1:])
        self.total_tokens = int(start[-1])
        self.host_tok_start = start
        flat = np.concatenate(parts)
        self.max_id, self.max_len = int(flat.max()), int(self.token_counts.max())
        if self.max_id >= (1 << 31):
            raise ValueError(f'ResidentText: the id {self.max_id} does not fit 32 bits')
        self.host_positions = (np.arange(self.total_tokens, dtype=np.int64) - np.repeat(start[:-1], self.token_counts)).astype(np.int32)
        self.host_ids = flat.astype(np.int32)
        self.ids = self.positions = self.tok_start = self.lengths = self.doc_sentences = None
        if self.device.type != 'cuda':
            return
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(self.device)
        self.ids, self.positions, self.tok_start = up(self.host_ids), up(self.host_positions), up(start)
        self.lengths, self.doc_sentences = up(self.token_counts.astype(np.int32)), up(self.sentences)

    def __len__(self):
        return self.n_docs

    @property
    def nbytes(self):
        """bytes of the resident tables; 0 on a CPU device"""
        return sum(t.numel() * t.element_size() for t in (self.ids, self.positions, self.tok_start, self.lengths, self.doc_sentences) if t is not None)

    # ---- the encoder pass (csrc/text_encoder.hip, wav2vec2.encoder_layers) -----------------------------------------------------------
    def _chunks(self, who, weights, out_dtype, workspace_bytes, attn):
        """the checks of the two passes, all before any launch, and the chunking -> [(a, b, attn)]: sentences a .. b - 1 go through the
        encoder together with that attention kernel; a chunk's activations stay within ``workspace_bytes`` (one sentence at the least)
        and within the 32-bit row indexing of mts_full_attn_fwd"""
        if not isinstance(weights, TextEncoderWeights):
            raise ValueError(f'{who}: weights must be a TextEncoderWeights (TextEncoderWeights.from_state_dict)')
        if out_dtype not in (torch.float32, torch.bfloat16):
            raise ValueError(f'{who}: out_dtype is torch.float32 or torch.bfloat16, not {out_dtype}')
        if attn not in ('auto', 'sentence', 'full'):
            raise ValueError(f"{who}: attn is 'auto', 'sentence' or 'full', not {attn!r}")
        if self.max_id >= weights.vocab_size:
            raise ValueError(f'{who}: the corpus holds the token id {self.max_id}, the vocabulary has {weights.vocab_size} rows')
        if weights.position_offset + self.max_len > weights.max_position_embeddings:
            raise ValueError(f'{who}: the longest sentence has {self.max_len} tokens; with position offset {weights.position_offset} the '
                             f'{weights.max_position_embeddings} rows of the position table allow '
                             f'{weights.max_position_embeddings - weights.position_offset} (truncate when tokenising)')
        if attn == 'sentence' and not weights.sent_attn_covers(self.max_len):
            raise NotImplementedError(f"{who}: attn='sentence' needs bf16 weights, a head dim that is a multiple of 32 up to 128 and sentences of at "
                                      f'most {SENT_ATTN_MAX_LEN} tokens; got {weights.dtype}, head dim {weights.hidden_size // weights.num_heads} and '
                                      f"{self.max_len} tokens (attn='full' or 'auto' serve them)")
        if self.device.type != 'cuda':
            raise RuntimeError(f'ResidentText.{who} runs on the GPU (there is no CPU fallback)')
        if weights.device != self.device:
            raise ValueError(f'{who}: the weights live on {weights.device}, the text on {self.device}')
        e = 2 if weights.dtype == torch.bfloat16 else 4
        per_token = e * (9 * weights.hidden_size + weights.intermediate_size) + 4 * weights.hidden_size + 4 * (weights.num_heads + 2) + 16
        budget = int(workspace_bytes if workspace_bytes is not None else self.WORKSPACE)
        rows_cap = ((1 << 31) - 1) // (3 * weights.hidden_size)        # n_sent * longest sentence of a chunk: what mts_full_attn_fwd indexes
        n, counts = self.total_sentences, self.token_counts
        chunks, a = [], 0
        while a < n:
            b, used, longest = a, 0, 0
            while b < n:
                longest_b = max(longest, int(counts[b]))
                if b > a and (used + int(counts[b]) * per_token > budget or (b - a + 1) * longest_b > rows_cap):
                    break
                used, longest, b = used + int(counts[b]) * per_token, longest_b, b + 1
            kernel = 'sentence' if attn == 'sentence' or (attn == 'auto' and weights.sent_attn_covers(longest)) else 'full'
            chunks.append((a, b, kernel))
            a = b
        return chunks

    def _forward(self, w, a, b, attn, out=None):
        """sentences a .. b - 1 through the encoder -> (their [tokens, H] last hidden states in the weights' dtype, the chunk's int64
        token table from 0)"""
        from . import ops
        from .wav2vec2 import encoder_layers
        ta, tb = int(self.host_tok_start[a]), int(self.host_tok_start[b])
        local = self.tok_start[a:b + 1] - ta
        pos = self.positions[ta:tb] + w.position_offset if w.position_offset else self.positions[ta:tb]
        direct = out is not None and w.num_layers == 0
        cur = out if direct else torch.empty((tb - ta, w.hidden_size), dtype=w.dtype, device=self.device)
        ops.text_embed(self.ids[ta:tb], pos, w.word, w.position, w.type_row, w.emb_gamma, w.emb_beta, w.eps, cur)
        y = encoder_layers(w.layers, cur, self.lengths[a:b], local[:-1].to(torch.int32), b - a, int(self.token_counts[a:b].max()), w.num_heads, w.eps,
                           out=out, attn=attn)
        return y, local

    def token_states(self, weights, out_dtype=torch.float32, workspace_bytes=None, attn='auto'):
        """-> ``frames.ResidentFrames`` of width ``weights.hidden_size`` on the device: ``last_hidden_state`` of every sentence, each
        encoded as a sequence of its own.  Sentence s owns its token rows and the sentence table is this text's, so ``pool(mode)`` and
        ``ResidentCorpus.with_frames(frames, 'mean', field)`` work unchanged.  The states are made a chunk of sentences at a time: a
        chunk's activations stay within ``workspace_bytes`` (default 1 GiB), only the [total_tokens, H] result is kept.  ``attn``: the
        attention kernel, 'sentence' (mts_sent_attn_fwd: bf16 weights, sentences up to 64 tokens; NotImplementedError elsewhere) |
        'full' (mts_full_attn_fwd) | 'auto' (per chunk, the sentence kernel where it covers: 0.72 x the full kernel's time on sentences of
        4 .. 60 tokens).  ValueError before any launch for a token
        id the vocabulary lacks and for a sentence longer than the position table allows; RuntimeError on a CPU device."""
        from . import ops
        chunks = self._chunks('token_states', weights, out_dtype, workspace_bytes, attn)
        out = torch.empty((self.total_tokens, weights.hidden_size), dtype=out_dtype, device=self.device)
        with torch.cuda.device(self.device):
            for a, b, kernel in chunks:
                dst = out[int(self.host_tok_start[a]):int(self.host_tok_start[b])]
                if out_dtype == weights.dtype:
                    self._forward(weights, a, b, kernel, out=dst)
                else:
                    y, local = self._forward(weights, a, b, kernel)
                    ops.w2v_rows(y, local[:-1].contiguous(), local, dst)
        return ResidentFrames.from_device(out, self.tok_start, self.sentences)

    def encode(self, weights, pooling='mean', out_dtype=torch.float32, workspace_bytes=None, attn='auto'):
        """-> [total_sentences, H] on the device in ``out_dtype``: the sentence embeddings, pooled chunk by chunk without keeping the token
        states.  ``pooling``: 'mean' (sentence-transformers' mean pooling over the sentence's tokens), 'cls' (the first token's state) or
        'max'.  No L2 normalisation is applied.  ``attn`` and the refusals as for ``token_states``."""
        if pooling not in POOLINGS:
            raise ValueError(f'encode: pooling is one of {POOLINGS}, not {pooling!r}')
        from . import ops
        chunks = self._chunks('encode', weights, out_dtype, workspace_bytes, attn)
        pooled = torch.empty((self.total_sentences, weights.hidden_size), dtype=out_dtype, device=self.device)
        with torch.cuda.device(self.device):
            for a, b, kernel in chunks:
                y, local = self._forward(weights, a, b, kernel)
                if pooling == 'cls':
                    ops.w2v_rows(y, local[:-1].contiguous(), torch.arange(b - a + 1, dtype=torch.int64, device=self.device), pooled[a:b])
                else:
                    ops.frame_pool(y, local, pooled[a:b], first=pooling)
                del y
        return pooled
