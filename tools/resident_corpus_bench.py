#!/usr/bin/env python3
"""What the device-resident corpus costs and what it saves (resident.ResidentCorpus, csrc/gather.hip; DESIGN.md §3 "Device-resident
corpus").  One process, every leg warmed, the legs taken IN TURN so that a drift of the machine hits all of them; REPS repetitions,
the report gives each repetition and the spread.

(a) the gather alone, every call between two device events, at BASELINE configs[1]'s batch 64 x 256 x 1792: equal lengths (256) and
    ragged lengths U{64..256} padded to 256, bf16 -> bf16 and fp32 -> bf16, out of a corpus of 256 documents with a fresh random index
    list per call.  Rate = (bytes read + bytes written) / time, next to a device copy (torch's copy_ kernel) of the same batch bytes and
    next to the repository's own Adam kernel (30 bytes per element with the bf16 mirror) in the same loop.
(b) NativeTrainer.step of the configs[1] transformer (bf16), a host clock round windows of steps that end in a synchronise, fed by
    (i)   one fixed batch resident in HBM, fp32 (bench.py's `value`), and (i') the same in bf16;
    (ii)  AudioPortionDataset(pin_memory=True, wire_dtype='bf16') -> DevicePrefetcher: the fastest pipeline without a resident corpus;
    (iii) ResidentCorpus(wire_dtype='bf16') + DocumentShardSampler: a new batch gathered on the device every step.

  python tools/resident_corpus_bench.py [--out profiles/resident_corpus_bench.txt] [--iters 200] [--steps 150] [--reps 3]

--segments runs the legs of segment-order augmentation INSTEAD (DESIGN.md §3 "Segment-order augmentation"; out: profiles/
segment_augment_bench.txt), same rules:
(a) mts_gather_pad and mts_gather_segments alone at 64 x 256 x 1792 bf16 out of 256 documents of 256 rows whose segments are about 20 rows
    long (a 5 % boundary rate): the plain gather, the segment gather with every segment in place, and with the 'shuffle' orders of
    AugmentedCorpus; a fresh index list and fresh tables per call, uploaded beforehand.  Both kernels move the same bytes.
(b) NativeTrainer.step of the configs[1] transformer fed by ResidentCorpus + sampler and by AugmentedCorpus('shuffle') + its sampler, and
    the host half of one augmented batch (drawing the orders, building the tables) timed on its own.

--mask runs the legs of negative-sentence masking INSTEAD (DESIGN.md §3 "Negative-sentence masking"; out: profiles/mask_inner_bench.txt),
same rules: the launches of one late-fusion batch of 64 documents of 256 rows (1792 + 1792 bf16 and the targets) -- mts_mask_plan and
three mts_gather_rows at keep probability 0.9 and 1.0 -- next to the plain batch's three mts_gather_pad of the same kind of index list,
in microseconds and as a ratio to the plain batch; the plan kernel alone; the host half of a masked batch and MaskedCorpus.set_epoch.
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from multimodaltopicsegmentation_amd import AudioPortionDataset, DevicePrefetcher, ResidentCorpus, ops  # noqa: E402
from multimodaltopicsegmentation_amd.taggers import Transformer_segmenter  # noqa: E402
from multimodaltopicsegmentation_amd.trainer import NativeTrainer  # noqa: E402

B, L, D, N_DOCS = 64, 256, 1792, 256
ADAM_N, ADAM_BYTES = 16 * 2 ** 20, 30
DEV = 'cuda'


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def gather_legs(iters, reps, say):
    g = torch.Generator().manual_seed(1)
    lengths = {'equal': torch.full((N_DOCS,), L, dtype=torch.int64), 'ragged': torch.randint(64, L + 1, (N_DOCS,), generator=g)}
    legs, nbytes = {}, {}
    for shape, ln in lengths.items():
        start = torch.zeros(N_DOCS + 1, dtype=torch.int64)
        start[1:] = ln.cumsum(0)
        total = int(start[-1])
        row_start = start.to(DEV)
        for src in (torch.bfloat16, torch.float32):
            corpus = torch.randn(total, D, device=DEV, dtype=torch.float32).to(src)
            dst = torch.empty(B, L, D, dtype=torch.bfloat16, device=DEV)
            lists = torch.randint(0, N_DOCS, (iters + 8, B), generator=g)
            idx_dev = lists.to(torch.int32).to(DEV)
            name = f'gather {"bf16" if src == torch.bfloat16 else "fp32"} -> bf16, {shape}'
            read = ln[lists].sum(1).double().mean().item() * D * corpus.element_size()         # mean over the index lists
            nbytes[name] = read + B * L * D * 2
            legs[name] = (lambda k, c=corpus, r=row_start, i=idx_dev, d=dst: ops.gather_pad(c, r, i[k % i.shape[0]], d))
    a16, b16 = torch.randn(B, L, D, device=DEV).to(torch.bfloat16), torch.empty(B, L, D, dtype=torch.bfloat16, device=DEV)
    a32 = torch.randn(B, L, D, device=DEV)
    legs['device copy bf16 -> bf16'] = lambda k: b16.copy_(a16)
    nbytes['device copy bf16 -> bf16'] = 2 * B * L * D * 2
    legs['device copy fp32 -> bf16'] = lambda k: b16.copy_(a32)
    nbytes['device copy fp32 -> bf16'] = B * L * D * 6
    p, gr, m, v = (torch.randn(ADAM_N, device=DEV) * s for s in (1.0, 1e-3, 1e-3, 0.0))
    v.abs_()
    mirror = torch.empty(ADAM_N, dtype=torch.bfloat16, device=DEV)
    legs['adam_step (16 Mi elements, bf16 mirror)'] = lambda k: ops.adam_step(p, gr, m, v, 1e-3, 0.9, 0.999, 1e-7, k + 1, 1.0, mirror)
    nbytes['adam_step (16 Mi elements, bf16 mirror)'] = ADAM_BYTES * ADAM_N
    for k in range(8):                                                                      # warm every leg
        for f in legs.values():
            f(k)
    torch.cuda.synchronize()
    out = {name: [] for name in legs}
    for _ in range(reps):
        ev = {name: [] for name in legs}
        for k in range(iters):
            for name, f in legs.items():
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s.record()
                f(k)
                e.record()
                ev[name].append((s, e))
        torch.cuda.synchronize()
        for name in legs:
            out[name].append(median([s.elapsed_time(e) * 1e3 for s, e in ev[name]]))
    say(f'(a) one call between two device events, median of {iters} per repetition, the legs in turn; batch {B} x {L} x {D}')
    res = {}
    for name, us in out.items():
        rates = [nbytes[name] / (t * 1e-6) / 1e12 for t in us]
        say(f'  {name:42s} {nbytes[name] / 1e6:7.1f} MB   ' + '  '.join(f'{t:7.1f} us' for t in us) + '   ' + '  '.join(f'{r:5.2f}' for r in rates) + ' TB/s')
        res[name] = {'MB': round(nbytes[name] / 1e6, 1), 'us': [round(t, 1) for t in us], 'TBps': [round(r, 3) for r in rates]}
    return res


def step_legs(steps, warmup, reps, say):
    def model():
        return Transformer_segmenter(2, D, 256, num_layers=1, nheads=8, loss_fn='FocalLoss', window_size=30, compute_dtype='bf16', seed=1234).to(DEV)
    g = torch.Generator().manual_seed(4321)
    lines = [(torch.randn(L, D, generator=g), (torch.rand(L, generator=g) < 0.05).float().tolist(), f'doc{i}') for i in range(N_DOCS)]
    ds = AudioPortionDataset(lines, {'0': 0, '1': 1}, CRF=False, truncate=False, pin_memory=True, wire_dtype='bf16', pin_slots=4,
                             collate_threads=min(16, os.cpu_count() or 8))
    corpus = ResidentCorpus(ds, DEV, wire_dtype='bf16')
    sampler = corpus.sampler(B, seed=9)
    epoch = [0]

    def index_lists(n):
        got = 0
        while got < n:
            sampler.set_epoch(epoch[0])
            epoch[0] += 1
            for ix, pad_to in sampler:
                if got < n:
                    got += 1
                    yield ix, pad_to
    fixed = ds.collater(ds.__getitems__(list(range(B))))
    fixed16 = {k: (v.to(DEV) if isinstance(v, torch.Tensor) and v.is_floating_point() else v) for k, v in fixed.items()}
    fixed32 = dict(fixed16, src_tokens=fixed16['src_tokens'].float())
    torch.cuda.synchronize()
    trainers = {name: NativeTrainer(model(), lr=1e-3, optimizer='Adam') for name in ('i', "i'", 'ii', 'iii')}

    def feed(name, n):
        if name == 'i':
            return (fixed32 for _ in range(n))
        if name == "i'":
            return (fixed16 for _ in range(n))
        if name == 'ii':
            return DevicePrefetcher((ds.collater(ds.__getitems__(ix)) for ix, _ in index_lists(n)), DEV, depth=2)
        return (corpus.batch(ix, pad_to) for ix, pad_to in index_lists(n))
    label = {'i': '(i)   fixed resident batch, fp32', "i'": "(i')  fixed resident batch, bf16",
             'ii': '(ii)  pinned bf16 collater -> DevicePrefetcher', 'iii': '(iii) ResidentCorpus(bf16) + sampler'}
    ms = {name: [] for name in trainers}
    for _ in range(reps):
        for name, tr in trainers.items():
            t0 = None
            for k, batch in enumerate(feed(name, warmup + steps)):
                if k == warmup:
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                tr.step(batch)
            torch.cuda.synchronize()
            ms[name].append(1e3 * (time.perf_counter() - t0) / steps)
    say(f'(b) NativeTrainer.step, configs[1] transformer bf16 at {B} x {L} x {D}: ms per step over windows of {steps} steps '
        f'({warmup} warm-up steps each), the legs in turn, {reps} repetitions; corpus {N_DOCS} documents, {corpus.nbytes / 1e6:.0f} MB resident')
    for name in trainers:
        say(f'  {label[name]:48s} ' + '  '.join(f'{t:.4f}' for t in ms[name]) + f'   median {median(ms[name]):.4f}  spread {max(ms[name]) - min(ms[name]):.4f}')
    d_ii = [a - b for a, b in zip(ms['iii'], ms['ii'])]
    d_i = [a - b for a, b in zip(ms['iii'], ms['i'])]
    d_i16 = [a - b for a, b in zip(ms['iii'], ms["i'"])]
    say('  (iii) - (ii)  per repetition: ' + '  '.join(f'{1e3 * d:+.1f} us' for d in d_ii))
    say('  (iii) - (i)   per repetition: ' + '  '.join(f'{1e3 * d:+.1f} us' for d in d_i))
    say("  (iii) - (i')  per repetition: " + '  '.join(f'{1e3 * d:+.1f} us' for d in d_i16))
    return {k: [round(t, 4) for t in v] for k, v in ms.items()}


def _boundary_lines(g):
    lines = []
    for i in range(N_DOCS):
        y = (torch.rand(L, generator=g) < 0.05).float()
        y[-1] = 0.0                                                                          # the loader's rule
        lines.append((torch.randn(L, D, generator=g), y.tolist(), f'doc{i}'))
    return lines


def segment_gather_legs(corpus, iters, reps, say):
    """(a) of --segments: the three gathers in turn out of one resident corpus"""
    import numpy as np
    g = torch.Generator().manual_seed(1)
    view = corpus.augmented('shuffle', seed=5)
    lists = torch.randint(0, N_DOCS, (iters + 8, B), generator=g).numpy()
    dst = torch.empty(B, L, D, dtype=torch.bfloat16, device=DEV)

    def tables(ii, orders):
        ptr, dst_off, src_off, rows, _ = corpus._segment_tables(ii, orders, False)
        return [torch.from_numpy(np.ascontiguousarray(t)).to(torch.int32).to(DEV) for t in (ii, ptr, dst_off, src_off, rows)]
    in_place = [tables(ii, [np.arange(corpus.n_segments[d]) for d in ii]) for ii in lists]
    shuffled = [tables(ii, [view.order(N_DOCS + int(d))[0] for d in ii]) for ii in lists]
    # the same documents as ONE range each (no search to speak of): what the table walk in front of the first load costs
    whole = [[torch.from_numpy(np.ascontiguousarray(t)).to(torch.int32).to(DEV)
              for t in (ii, np.arange(B + 1), np.zeros(B, dtype=np.int64), np.zeros(B, dtype=np.int64), corpus.rows[ii])] for ii in lists]
    listed = sum(int(t[2].numel()) for t in shuffled) / len(shuffled)
    # every leg takes ANOTHER index list in the same trip, so that none finds the rows its predecessor has just pulled into the caches
    legs = {'mts_gather_pad': lambda k: ops.gather_pad(corpus.corpus, corpus.row_start, in_place[k % len(lists)][0], dst),
            'mts_gather_segments, segments in place': lambda k: ops.gather_segments(corpus.corpus, corpus.row_start, *in_place[(k + 3) % len(lists)], dst),
            "mts_gather_segments, 'shuffle' orders": lambda k: ops.gather_segments(corpus.corpus, corpus.row_start, *shuffled[(k + 5) % len(lists)], dst),
            'mts_gather_segments, one listed range per document': lambda k: ops.gather_segments(corpus.corpus, corpus.row_start, *whole[(k + 6) % len(lists)], dst),
            'mts_gather_pad, once more (last in the trip)': lambda k: ops.gather_pad(corpus.corpus, corpus.row_start, in_place[(k + 7) % len(lists)][0], dst)}
    nbytes = 2 * B * L * D * 2
    for k in range(8):                                                                      # warm every leg
        for f in legs.values():
            f(k)
    torch.cuda.synchronize()
    out = {name: [] for name in legs}
    for _ in range(reps):
        ev = {name: [] for name in legs}
        for k in range(iters):
            for name, f in legs.items():
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s.record()
                f(k)
                e.record()
                ev[name].append((s, e))
        torch.cuda.synchronize()
        for name in legs:
            out[name].append(median([s.elapsed_time(e) * 1e3 for s, e in ev[name]]))
    say(f'(a) one call between two device events, median of {iters} per repetition, the legs in turn; batch {B} x {L} x {D} bf16 -> bf16, '
        f'{listed / B:.1f} listed segments per document')
    res = {}
    for name, us in out.items():
        rates = [nbytes / (t * 1e-6) / 1e12 for t in us]
        say(f'  {name:42s} {nbytes / 1e6:7.1f} MB   ' + '  '.join(f'{t:7.1f} us' for t in us) + '   ' + '  '.join(f'{r:5.2f}' for r in rates) + ' TB/s')
        res[name] = {'MB': round(nbytes / 1e6, 1), 'us': [round(t, 1) for t in us], 'TBps': [round(r, 3) for r in rates]}
    spread = max(out['mts_gather_pad']) - min(out['mts_gather_pad'])
    for name in list(legs)[1:]:
        say(f'  {name} - mts_gather_pad per repetition: ' + '  '.join(f'{a - b:+.1f} us' for a, b in zip(out[name], out['mts_gather_pad']))
            + f'   (the plain gather\'s own spread: {spread:.1f} us)')
    return res


def segment_step_legs(corpus, steps, warmup, reps, say):
    """(b) of --segments: the step fed by the corpus and by its augmented view"""
    def model():
        return Transformer_segmenter(2, D, 256, num_layers=1, nheads=8, loss_fn='FocalLoss', window_size=30, compute_dtype='bf16', seed=1234).to(DEV)
    view = corpus.augmented('shuffle', seed=5)
    sources = {'plain': (corpus, corpus.sampler(B, seed=9)), 'augmented': (view, view.sampler(B, seed=9))}
    epoch = {name: 0 for name in sources}

    def items(name, n):
        got = 0
        sampler = sources[name][1]
        while got < n:
            sampler.set_epoch(epoch[name])
            epoch[name] += 1
            for item in sampler:
                if got < n:
                    got += 1
                    yield item
    trainers = {name: NativeTrainer(model(), lr=1e-3, optimizer='Adam') for name in sources}
    label = {'plain': 'ResidentCorpus(bf16) + sampler', 'augmented': "AugmentedCorpus('shuffle') + its sampler"}
    ms = {name: [] for name in sources}
    for _ in range(reps):
        for name, tr in trainers.items():
            t0 = None
            for k, item in enumerate(items(name, warmup + steps)):
                if k == warmup:
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                tr.step(sources[name][0].batch(*item))
            torch.cuda.synchronize()
            ms[name].append(1e3 * (time.perf_counter() - t0) / steps)
    say(f'(b) NativeTrainer.step, configs[1] transformer bf16 at {B} x {L} x {D}: ms per step over windows of {steps} steps '
        f'({warmup} warm-up steps each), the legs in turn, {reps} repetitions; corpus {N_DOCS} documents, {corpus.nbytes / 1e6:.0f} MB resident')
    for name in sources:
        say(f'  {label[name]:48s} ' + '  '.join(f'{t:.4f}' for t in ms[name]) + f'   median {median(ms[name]):.4f}  spread {max(ms[name]) - min(ms[name]):.4f}')
    say('  augmented - plain per repetition: ' + '  '.join(f'{1e3 * (a - b):+.1f} us' for a, b in zip(ms['augmented'], ms['plain'])))
    # the host half of a batch on its own (no GPU work): what the loop's host thread pays per step before it can launch anything
    host = {}
    for name, (src, _) in sources.items():
        todo = list(items(name, steps))
        t0 = time.perf_counter()
        for item in todo:
            src.host_fields(*item)
        host[name] = 1e6 * (time.perf_counter() - t0) / steps
    view.set_epoch(0)
    t0 = time.perf_counter()
    for d in range(N_DOCS):
        view.order(N_DOCS + d)
    draw = 1e6 * (time.perf_counter() - t0) / N_DOCS
    say(f'  host half of one batch (host_fields, no launch): plain {host["plain"]:.0f} us, augmented {host["augmented"]:.0f} us; '
        f'one \'shuffle\' draw (np.random.default_rng([seed, epoch, d]).permutation(K)) {draw:.1f} us, about {B // 2} per batch')
    return {'step_ms': {k: [round(t, 4) for t in v] for k, v in ms.items()}, 'host_us': {k: round(v, 1) for k, v in host.items()},
            'draw_us': round(draw, 1)}


def mask_legs(corpus, iters, reps, say):
    """--mask: the kernels of a masked late-fusion batch (mts_mask_plan + three mts_gather_rows) next to the plain batch's (three
    mts_gather_pad) of the same documents, and the two host halves"""
    import numpy as np
    from multimodaltopicsegmentation_amd.resident import mask_doc_seeds
    g = torch.Generator().manual_seed(1)
    lists = torch.randint(0, N_DOCS, (iters + 8, B), generator=g).numpy().astype(np.int64)
    D2 = int(corpus.corpus2.shape[1])
    big = {name: torch.empty(B * L * w, dtype=dt, device=DEV) for name, w, dt in (('a', D, torch.bfloat16), ('b', D2, torch.bfloat16), ('t', 1, torch.float32))}
    table, kept = torch.empty(B * L, dtype=torch.int32, device=DEV), torch.empty(B, dtype=torch.int32, device=DEV)

    def prepared(p):
        out = []
        for k, ii in enumerate(lists):
            seeds = mask_doc_seeds(5, k, N_DOCS, ii)
            Lmax = int(corpus._mask_plan_host(ii, seeds, p)[0].max())
            out.append((torch.from_numpy(ii).to(torch.int32).to(DEV), torch.from_numpy(seeds.view(np.int64).copy()).to(DEV), Lmax))
        return out
    prep = {0.9: prepared(0.9), 1.0: prepared(1.0)}

    def plain(k):
        idx = prep[1.0][k % len(lists)][0]
        ops.gather_pad(corpus.corpus, corpus.row_start, idx, big['a'].view(B, L, D))
        ops.gather_pad(corpus.corpus2, corpus.row_start, idx, big['b'].view(B, L, D2))
        ops.gather_pad(corpus.targets, corpus.row_start, idx, big['t'].view(B, L), pad_value=-1.0)

    def plan(p, k):
        idx, seeds, Lmax = prep[p][k % len(lists)]
        return idx, Lmax, ops.mask_plan(corpus.targets, corpus.row_start, idx, seeds, p, table[:B * Lmax].view(B, Lmax), kept)[0]

    def masked(p, k):
        idx, Lmax, rows = plan(p, k)
        ops.gather_rows(corpus.corpus, corpus.row_start, idx, rows, big['a'][:B * Lmax * D].view(B, Lmax, D))
        ops.gather_rows(corpus.corpus2, corpus.row_start, idx, rows, big['b'][:B * Lmax * D2].view(B, Lmax, D2))
        ops.gather_rows(corpus.targets, corpus.row_start, idx, rows, big['t'][:B * Lmax].view(B, Lmax), pad_value=-1.0)
    # every leg takes ANOTHER index list in the same trip, so that none finds the rows its predecessor has just pulled into the caches
    legs = {'plain batch: 3 x mts_gather_pad': plain,
            'masked p = 0.9: mts_mask_plan + 3 x mts_gather_rows': lambda k: masked(0.9, k + 3),
            'masked p = 1.0: mts_mask_plan + 3 x mts_gather_rows': lambda k: masked(1.0, k + 5),
            'mts_mask_plan alone, p = 0.9': lambda k: plan(0.9, k + 6),
            'plain batch, once more (last in the trip)': lambda k: plain(k + 7)}
    for k in range(8):                                                                      # warm every leg
        for f in legs.values():
            f(k)
    torch.cuda.synchronize()
    out = {name: [] for name in legs}
    for _ in range(reps):
        ev = {name: [] for name in legs}
        for k in range(iters):
            for name, f in legs.items():
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s.record()
                f(k)
                e.record()
                ev[name].append((s, e))
        torch.cuda.synchronize()
        for name in legs:
            out[name].append(median([s.elapsed_time(e) * 1e3 for s, e in ev[name]]))
    mean_L = sum(t[2] for t in prep[0.9]) / len(lists)
    say(f'(a) the launches of one batch between two device events, median of {iters} per repetition, the legs in turn; {B} documents of {L} rows, '
        f'{D} + {D2} bf16 and the targets; padded length at p = 0.9: {mean_L:.1f} on average')
    base = out['plain batch: 3 x mts_gather_pad']
    res = {}
    for name, us in out.items():
        say(f'  {name:54s} ' + '  '.join(f'{t:7.1f} us' for t in us) + '   ratio to the plain batch ' + '  '.join(f'{t / b:5.3f}' for t, b in zip(us, base)))
        res[name] = {'us': [round(t, 1) for t in us], 'ratio': [round(t / b, 3) for t, b in zip(us, base)]}
    say(f'  table bytes of a masked batch: 4 x {B} x Lmax written by the plan and read by each of the three gathers ({4 * B * L} B at Lmax = {L}) '
        f'next to {B * L * (2 * D + 2 * D2 + 4)} destination bytes; the plan reads 4 B per stored row ({4 * B * L} B)')
    # the host halves: what the loop's host thread pays per step before it can launch anything, and the epoch's plan
    view = corpus.masked(0.9, seed=5)
    t0 = time.perf_counter()
    for e in range(1, 6):
        view.set_epoch(e)
    per_epoch = 1e6 * (time.perf_counter() - t0) / 5
    host = {}
    for name, src in (('plain', corpus), ('masked', view)):
        t0 = time.perf_counter()
        for ii in lists[:iters]:
            src.host_fields(ii)
        host[name] = 1e6 * (time.perf_counter() - t0) / iters
    say(f'  host half of one batch (host_fields, no launch): plain {host["plain"]:.0f} us, masked {host["masked"]:.0f} us; '
        f'MaskedCorpus.set_epoch ({corpus.total_rows} sentences): {per_epoch:.0f} us per epoch')
    res['host_us'] = {k: round(v, 1) for k, v in host.items()}
    res['set_epoch_us'] = round(per_epoch, 1)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--mask', action='store_true', help='the legs of negative-sentence masking instead (mask_legs)')
    ap.add_argument('--segments', action='store_true', help='the legs of segment-order augmentation instead (module docstring)')
    ap.add_argument('--iters', type=int, default=200)
    ap.add_argument('--steps', type=int, default=150)
    ap.add_argument('--warmup', type=int, default=15)
    ap.add_argument('--reps', type=int, default=3)
    a = ap.parse_args()
    if a.out is None:
        a.out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles',
                             'mask_inner_bench.txt' if a.mask else 'segment_augment_bench.txt' if a.segments else 'resident_corpus_bench.txt')
    if not torch.cuda.is_available():
        sys.exit('resident_corpus_bench: no GPU visible; nothing is measured without one')
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    say(f'tools/resident_corpus_bench.py {"--mask " if a.mask else "--segments " if a.segments else ""}--iters {a.iters} --steps {a.steps} --warmup {a.warmup} --reps {a.reps}'
        f'   ({torch.cuda.get_device_name(0)})')
    if a.mask:
        ds = AudioPortionDataset(_boundary_lines(torch.Generator().manual_seed(4321)), {'0': 0, '1': 1}, CRF=False, truncate=False,
                                 second_input=_boundary_lines(torch.Generator().manual_seed(1234)))
        res = {'mask': mask_legs(ResidentCorpus(ds, DEV, wire_dtype='bf16'), a.iters, a.reps, say)}
    elif a.segments:
        ds = AudioPortionDataset(_boundary_lines(torch.Generator().manual_seed(4321)), {'0': 0, '1': 1}, CRF=False, truncate=False)
        corpus = ResidentCorpus(ds, DEV, wire_dtype='bf16')
        res = {'gather': segment_gather_legs(corpus, a.iters, a.reps, say)}
        res.update(segment_step_legs(corpus, a.steps, a.warmup, a.reps, say))
    else:
        res = {'gather': gather_legs(a.iters, a.reps, say)}
        res['step_ms'] = step_legs(a.steps, a.warmup, a.reps, say)
    say(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
