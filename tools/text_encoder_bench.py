#!/usr/bin/env python3
"""What on-device BERT / RoBERTa sentence embeddings cost (text.py, csrc/text_encoder.hip; DESIGN.md "Text sentence features from resident
token ids") next to the host route a user had before, and what attention takes of a layer with each of its two kernels.  One process,
random weights at the base size (12 layers, hidden 768, 12 heads, intermediate 3072, vocabulary 50 265) in bf16, --sentences synthetic
sentences with lengths uniform in 4 .. 60 (leg 1) and 4 .. 128 (leg 2) from a fixed seed; every leg warmed, the legs of a repetition run
one after another (interleaved), median and spread (min .. max) over --reps repetitions.

(a) ``text.encode(weights, 'mean')`` end to end with attn='auto' and attn='full': a host clock round work that ends in a device
    synchronise;
(b) one chunk (the first the default workspace gives) per stage between device events, each window --inner launches long: the embedding
    stage, one layer's four GEMMs, its two LayerNorms, and its attention on the SAME qkv with ``mts_sent_attn_fwd`` and with
    ``mts_full_attn_fwd``; attention's share of the layer's time follows for each kernel;
(c) the host route: ``transformers``' ``RobertaModel`` on the CPU at batch size 1 for --host-sentences sentences, SCALED to the corpus by
    tokens (only where ``transformers`` imports; --host-sentences 0 skips it).

  python tools/text_encoder_bench.py [--out profiles/text_encoder_bench.json] [--reps 7] [--sentences 30000] [--host-sentences 16]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from multimodaltopicsegmentation_amd import ResidentText, TextEncoderWeights, ops  # noqa: E402

DEV = 'cuda'
BASE = dict(vocab=50265, hidden=768, heads=12, intermediate=3072, layers=12, positions=514, eps=1e-5)


def make_corpus(n_sent, lo, hi, seed, n_docs=8):
    g = np.random.default_rng([71, seed])
    lens = g.integers(lo, hi + 1, size=n_sent)
    cut = np.rint(np.linspace(0, n_sent, n_docs + 1)).astype(np.int64)
    return [[g.integers(3, BASE['vocab'], size=int(n)).tolist() for n in lens[a:b]] for a, b in zip(cut[:-1], cut[1:])]


def device_time(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner


def host_time(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def summary(xs):
    return {'median': statistics.median(xs), 'min': min(xs), 'max': max(xs), 'all': xs}


def leg(name, docs, w, reps, inner):
    text = ResidentText(docs, DEV)
    H, I, heads = w.hidden_size, w.intermediate_size, w.num_heads
    out = {'sentences': text.total_sentences, 'tokens': text.total_tokens, 'longest sentence': text.max_len}
    kinds = ('auto', 'full')
    chunks = text._chunks('encode', w, torch.float32, None, 'auto')
    out['chunks'] = len(chunks)
    out["chunks whose attention 'auto' gives to mts_sent_attn_fwd"] = sum(k == 'sentence' for _, _, k in chunks)
    for k in kinds:
        text.encode(w, 'mean', attn=k)
    e2e = {k: [] for k in kinds}
    for _ in range(reps):
        for k in kinds:
            e2e[k].append(host_time(lambda: text.encode(w, 'mean', attn=k)))
    out["text.encode(weights, 'mean') ms"] = {k: summary(v) for k, v in e2e.items()}
    med = statistics.median(e2e['auto'])
    out['auto: sentences per second'] = text.total_sentences / (med * 1e-3)
    flops = float(w.num_layers * (2 * (4 * H * H + 2 * H * I) * text.total_tokens + 4 * H * int((text.token_counts.astype(np.float64) ** 2).sum())))
    out['auto: TFLOP/s of the layers (multiply-adds x 2)'] = flops / (med * 1e-3) / 1e12

    # one chunk, stage by stage
    a, b, _ = chunks[0]
    ta, tb = int(text.host_tok_start[a]), int(text.host_tok_start[b])
    T, longest = tb - ta, int(text.token_counts[a:b].max())
    out['the chunk'] = {'sentences': b - a, 'tokens': T, 'longest sentence': longest}
    new = lambda *s: torch.empty(s, dtype=w.dtype, device=DEV)
    cur, qkv, ctx, s1, a1, u, s2 = new(T, H), new(T, 3 * H), new(T, H), new(T, H), new(T, H), new(T, I), new(T, H)
    mean, rstd = (torch.empty(T, dtype=torch.float32, device=DEV) for _ in range(2))
    lse = torch.empty((T, heads), dtype=torch.float32, device=DEV)
    lengths, row0 = text.lengths[a:b], (text.tok_start[a:b] - ta).to(torch.int32)
    ids, pos = text.ids[ta:tb], text.positions[ta:tb] + w.position_offset
    p = w.layers[0]

    def gemms():
        ops.linear_fwd(cur, p['qkv_w'], p['qkv_b'], qkv, colscale=float(H // heads) ** -0.5, ncols_scaled=H)
        ops.linear_fwd(ctx, p['o_w'], p['o_b'], s1, residual=cur)
        ops.linear_fwd(a1, p['ff1_w'], p['ff1_b'], u, gelu=True)
        ops.linear_fwd(u, p['ff2_w'], p['ff2_b'], s2, residual=a1)

    def norms():
        ops.layernorm_fwd(s1, p['ln1_g'], p['ln1_b'], w.eps, a1, mean, rstd)
        ops.layernorm_fwd(s2, p['ln2_g'], p['ln2_b'], w.eps, s1, mean, rstd)

    legs = {'embedding stage (mts_text_embed)': lambda: ops.text_embed(ids, pos, w.word, w.position, w.type_row, w.emb_gamma, w.emb_beta, w.eps, cur),
            "one layer's four GEMMs": gemms, "one layer's two LayerNorms": norms,
            'attention: mts_full_attn_fwd': lambda: ops.full_attn_fwd(qkv, lengths, b - a, longest, H, heads, ctx, lse, row0=row0)}
    if w.sent_attn_covers(longest):
        legs['attention: mts_sent_attn_fwd'] = lambda: ops.sent_attn_fwd(qkv, row0, lengths, longest, H, heads, ctx)
    legs['embedding stage (mts_text_embed)']()
    ops.layernorm_fwd(cur, p['ln1_g'], p['ln1_b'], w.eps, a1, mean, rstd)          # finite operands for every leg
    ctx.copy_(cur), s1.copy_(cur), s2.copy_(cur)
    for fn in legs.values():
        fn()
    torch.cuda.synchronize()
    times = {k: [] for k in legs}
    for _ in range(reps):
        for k, fn in legs.items():
            times[k].append(device_time(fn, inner))
    out['stages of the chunk, ms'] = {k: summary(v) for k, v in times.items()}
    m = {k: statistics.median(v) for k, v in times.items()}
    rest = m["one layer's four GEMMs"] + m["one layer's two LayerNorms"]
    out["attention's share of a layer's time"] = {k.split(': ')[1]: m[k] / (rest + m[k]) for k in m if k.startswith('attention')}
    out['attention GFLOP of the chunk (4 H sum len^2)'] = 4.0 * H * float((text.token_counts[a:b].astype(np.float64) ** 2).sum()) / 1e9
    out["attention's share of a layer's FLOPs"] = 4.0 * H * float((text.token_counts[a:b].astype(np.float64) ** 2).sum()) / (
        2.0 * (4 * H * H + 2 * H * I) * T + 4.0 * H * float((text.token_counts[a:b].astype(np.float64) ** 2).sum()))
    if 'attention: mts_sent_attn_fwd' in m:
        s, f = times['attention: mts_sent_attn_fwd'], times['attention: mts_full_attn_fwd']
        out['sentence kernel median / full kernel median'] = m['attention: mts_sent_attn_fwd'] / m['attention: mts_full_attn_fwd']
        out['full median - sentence median, ms'] = m['attention: mts_full_attn_fwd'] - m['attention: mts_sent_attn_fwd']
        out['the two spreads together (max - min of each), ms'] = (max(s) - min(s)) + (max(f) - min(f))
    return name, out, text


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--inner', type=int, default=10)
    ap.add_argument('--sentences', type=int, default=30000)
    ap.add_argument('--host-sentences', type=int, default=16)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('text_encoder_bench: no GPU visible; nothing is measured on the CPU')
    from tests import text_encoder_oracle as TO
    sd = TO.random_state_dict(BASE, 1)
    w = TextEncoderWeights.from_state_dict(sd, TO.config_dict(BASE, 'roberta'), device=DEV, dtype='bf16')
    report = {'device': torch.cuda.get_device_name(0), 'reps': a.reps, 'launches per device-event window': a.inner, 'dtype': 'bf16',
              'size': {k: v for k, v in BASE.items()}}
    texts = {}
    for name, lo, hi, seed in (('leg 1: lengths 4..60', 4, 60, 0), ('leg 2: lengths 4..128', 4, 128, 1)):
        docs = make_corpus(a.sentences, lo, hi, seed)
        name, out, texts[name] = leg(name, docs, w, a.reps, a.inner)
        report[name] = out
        texts[name + ' docs'] = docs

    if a.host_sentences > 0:
        try:
            import transformers as tr
        except Exception:  # noqa: BLE001
            tr = None
        if tr is not None:
            torch.set_num_threads(16)
            hc = tr.RobertaConfig(vocab_size=BASE['vocab'], max_position_embeddings=BASE['positions'], hidden_dropout_prob=0.0,
                                  attention_probs_dropout_prob=0.0)
            model = tr.RobertaModel(hc).eval()
            docs = texts['leg 1: lengths 4..60 docs']
            flat = [torch.tensor(s) for d in docs for s in d]
            pick = np.random.default_rng(7).choice(len(flat), size=min(a.host_sentences, len(flat)), replace=False).tolist()
            with torch.no_grad():
                model(input_ids=flat[pick[0]][None])
                t = time.perf_counter()
                for i in pick:
                    model(input_ids=flat[i][None]).last_hidden_state.mean(dim=1)
                sec = time.perf_counter() - t
            n = int(sum(flat[i].shape[0] for i in pick))
            total = texts['leg 1: lengths 4..60'].total_tokens
            report['host route (transformers %s RobertaModel, CPU fp32, batch 1; threads %s), leg 1' % (tr.__version__, torch.get_num_threads())] = {
                'sentences': len(pick), 'tokens': n, 'seconds': sec, 'seconds SCALED to the corpus by tokens': sec * total / n}
    text = json.dumps(report, indent=1)
    print(text)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
