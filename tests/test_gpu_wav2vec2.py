"""GPU checks of the wav2vec 2.0 path (csrc/wav2vec2.hip, wav2vec2.py, ResidentAudio.wav2vec2) against the fp64 restatement of
tests/wav2vec2_oracle.py (itself checked against ``transformers`` in tests/test_wav2vec2_cpu.py).

The stage tests are STAGED: every stage is checked given the DEVICE's output of the stage before it, so one stage's error is not charged to
the next.  Tolerances are not fixed numbers: with ``e_dev`` the device's max abs error against the fp64 oracle and ``e_ref`` that of the same
restatement run by torch on the CPU in the device's dtype (fp32; or fp32 with the matrices and every stored activation rounded to bf16),
every comparison requires ``e_dev <= 4 e_ref + 4 eps(dtype) max|oracle|`` (``wav2vec2_oracle.within``, which prints the figures).  The
factor 4 covers another summation order and other rounding points; a wrong tap, frame offset, group or sentence gives errors of the size
of the values themselves.

Small configuration (every kernel path is the real one: matrix-core attention at head dim 32, H / G = 32, an even positional kernel):
conv_dim 32 x 7 at the default kernels and strides, hidden 128, 4 heads, intermediate 256, 2 layers, K_p = 16, G = 4.  Sentences: two
documents of 400, 719, 720 and 16 000, 49 999, 4 001 samples (1, 1, 2, 49, 155, 12 frames): the one- and two-frame sentences, the floor
edge, one sentence beyond a 64-frame tile of the positional convolution and of attention, ragged block bases.  Sentence 3 carries a
constant offset of 3.0, so the utterance normalisation matters."""
import numpy as np
import pytest
import torch

from tests import wav2vec2_oracle as WO
from tests.test_pca_cpu import corpus_of

pytestmark = pytest.mark.gpu
DEV = 'cuda'
LENGTHS = [400, 719, 720, 16000, 49999, 4001]
DOCS = [3, 3]
EPS = {'fp32': 2.0 ** -23, 'bf16': 2.0 ** -7}
_CACHE = {}


def _sd():
    if 'sd' not in _CACHE:
        _CACHE['sd'] = WO.random_state_dict(WO.SMALL, 7)
    return _CACHE['sd']


def _oracle(mode, cfg=WO.SMALL, sd=None):
    key = ('oracle', mode, id(cfg))
    if sd is not None:
        return WO.Oracle(sd, cfg, mode)
    if key not in _CACHE:
        _CACHE[key] = WO.Oracle(_sd(), cfg, mode)
    return _CACHE[key]


def _weights(dtype, sd=None, cfg=WO.SMALL):
    from multimodaltopicsegmentation_amd import Wav2Vec2Weights
    if sd is not None:
        return Wav2Vec2Weights.from_state_dict(sd, WO.hf_config_dict(cfg), device=DEV, dtype=dtype)
    if ('w', dtype) not in _CACHE:
        _CACHE['w', dtype] = Wav2Vec2Weights.from_state_dict(_sd(), WO.hf_config_dict(cfg), device=DEV, dtype=dtype)
    return _CACHE['w', dtype]


def _audio(sents, docs=DOCS, **kw):
    """ResidentAudio over sentences laid one after another in their documents"""
    from multimodaltopicsegmentation_amd import ResidentAudio
    waves, spans, i = [], [], 0
    for n in docs:
        part = sents[i:i + n]
        edges = np.concatenate([[0], np.cumsum([len(p) for p in part])])
        waves.append(torch.cat(part).numpy())
        spans.append([(int(a), int(b)) for a, b in zip(edges[:-1], edges[1:])])
        i += n
    return ResidentAudio(waves, spans, DEV, unit='samples', min_samples=400, **kw)


def _sents(seed=0):
    if ('sents', seed) not in _CACHE:
        _CACHE['sents', seed] = WO.signals(LENGTHS, seed=seed, offset_at=3)
    return _CACHE['sents', seed]


def _per_sentence(fn, rows, counts):
    """fn on every sentence's own rows of a stacked matrix -> the stacked results"""
    out, a = [], 0
    for n in counts:
        out.append(fn(rows[a:a + int(n)]))
        a += int(n)
    return torch.cat(out)


@pytest.mark.parametrize('dtype', ['fp32', 'bf16'])
def test_stage_by_stage_against_the_oracle(dtype):
    from multimodaltopicsegmentation_amd import ops, wav2vec2 as W
    w, sents, audio = _weights(dtype), _sents(), _audio(_sents())
    O, R, eps = _oracle('fp64'), _oracle(dtype), EPS[dtype]
    plan = W.ChunkPlan(audio.sample_counts, w, audio.device)
    assert plan.frames.tolist() == [1, 1, 2, 49, 155, 12] and plan.rows0 % 64 == 0 and (plan.block_start % 64 == 0).all()

    # utterance statistics (always fp32 on the device)
    stats = ops.w2v_wave_stats(audio.wave, audio.sent_start, audio.sent_len).cpu()
    want = torch.tensor([[float(v) for v in O.wave_stats(x.double())] for x in sents], dtype=torch.float64)
    ref = torch.tensor([[float(v) for v in _oracle('fp32').wave_stats(x)] for x in sents])
    WO.within(stats, want, ref, EPS['fp32'], 'wave_stats')

    # conv layer 0 + group norm + GELU, then every conv GEMM layer given the device's layer before it (the lda < K check, both dtypes)
    bufs = W.conv_features(w, audio.wave, audio.sent_start, audio.sent_len, plan, keep=True)
    torch.cuda.synchronize()
    x0 = plan.valid_rows(bufs[0], 0).cpu()
    WO.within(x0, torch.cat([O.conv0(x.double()) for x in sents]), torch.cat([R.conv0(x) for x in sents]), eps, f'conv0 {dtype}')
    keep = torch.zeros(plan.rows0 + W.SLACK, dtype=torch.bool)
    for b, t in zip(plan.block_start[:-1], plan.T[0]):
        keep[int(b):int(b) + int(t)] = True
    assert not bool(bufs[0].cpu()[~keep].any()), 'rows of a block behind its sentence, and the slack rows, are zero'
    for l in range(1, plan.n_layers):
        prev = plan.valid_rows(bufs[l - 1], l - 1).cpu()
        got = plan.valid_rows(bufs[l], l).cpu()
        assert bool(torch.isfinite(bufs[l][:plan.rows0 >> l].float()).all()), 'rows between the blocks are computed, and finite'
        WO.within(got, _per_sentence(lambda r: O.conv(l, r.double()), prev, plan.T[l - 1]),
                  _per_sentence(lambda r: R.conv(l, r.float()), prev, plan.T[l - 1]), eps, f'conv layer {l} {dtype}')
    # the two alternating buffers of the product path give the same bits as one buffer per layer
    top = W.conv_features(w, audio.wave, audio.sent_start, audio.sent_len, plan)
    last = plan.n_layers - 1
    assert torch.equal(plan.valid_rows(top, last), plan.valid_rows(bufs[last], last))

    # feature projection
    h = W.project(w, bufs[last], plan)
    top_rows = plan.valid_rows(bufs[last], last).cpu()
    h_rows = plan.valid_rows(h, last).cpu()
    WO.within(h_rows, _per_sentence(lambda r: O.project(r.double()), top_rows, plan.frames),
              _per_sentence(lambda r: R.project(r.float()), top_rows, plan.frames), eps, f'projection {dtype}')

    # regroup, bitwise: the padded rows are zero and the valid rows equal
    y_gemm, xg = W.pos_conv_gemm(w, h, plan, keep=True)
    G, Kp, H = w.pos_groups, w.pos_kernel, w.hidden_size
    expect = torch.zeros((plan.rows_p, H), dtype=w.dtype)
    for s in range(plan.n_sent):
        a = int(plan.pad_start[s]) + Kp // 2
        expect[a:a + int(plan.frames[s])] = h.cpu()[int(plan.block_start[s]) >> last:(int(plan.block_start[s]) >> last) + int(plan.frames[s])]
    assert torch.equal(xg.cpu(), expect.view(plan.rows_p, G, H // G).permute(1, 0, 2).contiguous())

    # positional convolution: the GEMM form, the matrix-core kernel, each against the oracle and against each other
    want = _per_sentence(lambda r: O.pos_conv(r.double()), h_rows, plan.frames)
    ref = _per_sentence(lambda r: R.pos_conv(r.float()), h_rows, plan.frames)
    WO.within(y_gemm.cpu(), want, ref, eps, f'pos conv, GEMM form {dtype}')
    if dtype == 'bf16':
        assert W.pos_conv_kernel_covers(w)
        y_kernel = W.pos_conv_kernel(w, h, plan)
        WO.within(y_kernel.cpu(), want, ref, eps, 'pos conv, kernel bf16')
        e_ref = float((ref.double() - want).abs().max())
        between = float((y_kernel.double() - y_gemm.double()).abs().max())
        print(f'pos conv, kernel against GEMM form: {between:.3e}')
        assert between <= 4 * e_ref + 4 * eps * float(want.abs().max())
        assert torch.equal(y_kernel, W.pos_conv_kernel(w, h, plan))

    # the transformer on the compact rows, given the device's positional output
    out = W.transformer(w, y_gemm, plan).cpu()
    WO.within(out, _per_sentence(lambda r: O.encoder(r.double()), y_gemm.cpu(), plan.frames),
              _per_sentence(lambda r: R.encoder(r.float()), y_gemm.cpu(), plan.frames), eps, f'transformer {dtype}')


@pytest.mark.parametrize('dtype', ['fp32', 'bf16'])
def test_end_to_end_against_the_oracle(dtype):
    w, sents, audio = _weights(dtype), _sents(), _audio(_sents())
    total = sum(WO.frame_count(n) for n in LENGTHS)
    out = torch.full((total, w.hidden_size), float('nan'), dtype=torch.float32, device=DEV)
    frames = audio.wav2vec2(w, out=out)                            # from_device refuses a row that was left unwritten (NaN)
    assert frames.frames.data_ptr() == out.data_ptr() and frames.D == 128 and frames.sentences.tolist() == DOCS
    assert frames.frame_start.cpu().tolist() == np.concatenate([[0], np.cumsum([WO.frame_count(n) for n in LENGTHS])]).tolist()
    assert bool(torch.isfinite(out).all())
    O, R = _oracle('fp64'), _oracle(dtype)
    WO.within(out.cpu(), torch.cat([O.forward(x.double()) for x in sents]), torch.cat([R.forward(x) for x in sents]), EPS[dtype], f'end to end {dtype}')
    if dtype == 'bf16':                                            # the bf16 result is what the fp32 output holds; both forms of the pos conv run
        assert torch.equal(audio.wav2vec2(w, out_dtype=torch.bfloat16).frames.float(), out)
        other = audio.wav2vec2(w, pos='gemm').frames
        WO.within(other.cpu(), torch.cat([O.forward(x.double()) for x in sents]), torch.cat([R.forward(x) for x in sents]), EPS[dtype],
                  'end to end bf16, GEMM form of the pos conv')


def test_real_size_positional_convolution():
    """H = 768, G = 16, K_p = 128 in bf16; sentences of 49, 1 and 150 frames of random input"""
    from multimodaltopicsegmentation_amd import wav2vec2 as W
    cfg = dict(WO.BASE, layers=0)
    sd = WO.random_state_dict(cfg, 21)
    w = _weights('bf16', sd, cfg)
    counts = [16000, 400, 149 * 320 + 400]
    plan = W.ChunkPlan(counts, w, torch.device(DEV))
    assert plan.frames.tolist() == [49, 1, 150]
    last = plan.n_layers - 1
    h = torch.randn((plan.rows0 >> last, 768), generator=torch.Generator().manual_seed(2)).to(torch.bfloat16).to(DEV)
    y_kernel, y_gemm = W.pos_conv_kernel(w, h, plan), W.pos_conv_gemm(w, h, plan)
    rows = plan.valid_rows(h, last).cpu()
    O, R = _oracle('fp64', cfg, sd), _oracle('bf16', cfg, sd)
    want = _per_sentence(lambda r: O.pos_conv(r.double()), rows, plan.frames)
    ref = _per_sentence(lambda r: R.pos_conv(r.float()), rows, plan.frames)
    WO.within(y_kernel.cpu(), want, ref, EPS['bf16'], 'real-size pos conv, kernel')
    WO.within(y_gemm.cpu(), want, ref, EPS['bf16'], 'real-size pos conv, GEMM form')
    between = float((y_kernel.double() - y_gemm.double()).abs().max())
    print(f'real-size pos conv, kernel against GEMM form: {between:.3e}')
    assert between <= 4 * float((ref.double() - want).abs().max()) + 4 * EPS['bf16'] * float(want.abs().max())


def test_real_size_whole_pass():
    """the base configuration (12 layers) with random weights, three sentences of 1, 0.75 and 0.5 s, bf16"""
    cfg = WO.BASE
    sd = WO.random_state_dict(cfg, 22)
    w = _weights('bf16', sd, cfg)
    sents = WO.signals([16000, 12000, 8000], seed=5, offset_at=1)
    audio = _audio(sents, docs=[2, 1])
    got = audio.wav2vec2(w).frames.cpu()
    O, R = _oracle('fp64', cfg, sd), _oracle('bf16', cfg, sd)
    with torch.no_grad():
        WO.within(got, torch.cat([O.forward(x.double()) for x in sents]), torch.cat([R.forward(x) for x in sents]), EPS['bf16'], 'real-size whole pass')


@pytest.mark.parametrize('dtype', ['fp32', 'bf16'])
def test_sentences_are_isolated(dtype):
    w, sents = _weights(dtype), _sents()
    audio = _audio(sents)
    base = audio.wav2vec2(w)
    start = base.frame_start.cpu().tolist()
    assert torch.equal(base.frames, audio.wav2vec2(w).frames), 'two calls with the same inputs are bitwise equal'
    other = WO.signals(LENGTHS, seed=99, offset_at=0)
    for k in (1, 4):                                               # neighbours replaced, block bases unchanged: the same bits
        mixed = [sents[i] if i == k else 2.0 * other[i] for i in range(len(LENGTHS))]
        got = _audio(mixed).wav2vec2(w).frames
        assert torch.equal(got[start[k]:start[k + 1]], base.frames[start[k]:start[k + 1]]), k
        assert not torch.equal(got[start[k + 1]:start[k + 1] + 1], base.frames[start[k + 1]:start[k + 1] + 1])
    O, R = _oracle('fp64'), _oracle(dtype)
    for k in (0, 4):                                               # alone: another GEMM shape, so the rule and not the bits
        alone = _audio([sents[k]], docs=[1]).wav2vec2(w).frames.cpu()
        want, ref = O.forward(sents[k].double()), R.forward(sents[k])
        WO.within(alone, want, ref, EPS[dtype], f'sentence {k} alone {dtype}')
        inside = base.frames[start[k]:start[k + 1]].cpu()
        between = float((alone.double() - inside.double()).abs().max())
        print(f'sentence {k} alone against in the batch: {between:.3e} (bitwise: {torch.equal(alone, inside)})')
        assert between <= 4 * float((ref.double() - want).abs().max()) + 4 * EPS[dtype] * float(want.abs().max())
    # one sentence per chunk
    from multimodaltopicsegmentation_amd import wav2vec2 as W
    _, chunks = audio._w2v_chunks('wav2vec2', w, torch.float32, 1)
    assert chunks == [(i, i + 1) for i in range(len(LENGTHS))]
    _, chunks = audio._w2v_chunks('wav2vec2', w, torch.float32, int(W.chunk_bytes(w, audio.sample_counts)[:3].sum()))
    assert chunks[0] == (0, 3)
    single = audio.wav2vec2(w, workspace_bytes=1)
    assert torch.equal(single.frame_start, base.frame_start)
    want, ref = torch.cat([O.forward(x.double()) for x in sents]), torch.cat([R.forward(x) for x in sents])
    WO.within(single.frames.cpu(), want, ref, EPS[dtype], f'one sentence per chunk {dtype}')
    between = float((single.frames.double() - base.frames.double()).abs().max())
    print(f'one sentence per chunk against one chunk: {between:.3e}')
    assert between <= 4 * float((ref.double() - want).abs().max()) + 4 * EPS[dtype] * float(want.abs().max())


def test_interface():
    from multimodaltopicsegmentation_amd import ResidentAudio
    w, sents = _weights('bf16'), _sents()
    audio = _audio(sents)
    frames = audio.wav2vec2(w)
    for mode in ('mean', 'max', 'mean_std', 'max_std', 'last'):
        assert torch.equal(audio.wav2vec2_stats(w, mode), frames.pool(mode)), mode
        assert torch.equal(audio.wav2vec2_stats(w, mode, workspace_bytes=1), audio.wav2vec2(w, workspace_bytes=1).pool(mode)), mode
    assert frames.pool('delta_gap').shape == (6, 128)
    with pytest.raises(ValueError, match=r"delta_gap.*wav2vec2\(weights\).pool\('delta_gap'\)"):
        audio.wav2vec2_stats(w, 'delta_gap')
    # into a corpus: one batch compared
    rows = audio.sentences.tolist()
    text = np.ascontiguousarray(np.random.default_rng(5).integers(-8, 9, size=(sum(rows), 6)).astype(np.float32))
    fused = corpus_of(text, rows, DEV).with_frames(frames, 'mean_std', field='embeddings2')
    want = frames.pool('mean_std', out_dtype=fused.corpus2.dtype)
    assert torch.equal(fused.corpus2, want)
    b = fused.batch([1, 0])
    assert b['src_tokens2'].shape[2] == 256
    for i, d in enumerate((1, 0)):
        assert torch.equal(b['src_tokens2'][i, :3], want[3 * d:3 * d + 3])
    # refusals, with the document and the sentence named, before any launch
    short = [sents[0], sents[1][:399], sents[2], sents[3], sents[4], sents[5]]
    with pytest.raises(ValueError, match='sentence 1 of document 0 has 399 samples, fewer than the 400 that give one wav2vec 2.0 frame'):
        ResidentAudio([torch.cat(short[:3]).numpy(), torch.cat(short[3:]).numpy()],
                      [[(0, 400), (400, 799), (799, 1519)], [(0, 16000), (16000, 65999), (65999, 70000)]], DEV, unit='samples', min_samples=1).wav2vec2(w)
    bad = [s.clone() for s in sents]
    bad[4][77] = float('nan')
    with pytest.raises(ValueError, match=r'sample 16077 of document 1 \(in sentence 1\) is not finite'):
        _audio(bad)
    with pytest.raises(ValueError, match='weights live on cpu'):
        from multimodaltopicsegmentation_amd import Wav2Vec2Weights
        audio.wav2vec2(Wav2Vec2Weights.from_state_dict(_sd(), WO.hf_config_dict(WO.SMALL)))


def test_refused_calls_leave_the_output_untouched():
    """each MTS_ERR_INVALID / MTS_ERR_UNSUPPORTED case of the new entry points returns its code without touching the output"""
    from multimodaltopicsegmentation_amd import _lib as L
    sentinel = lambda n, dt=torch.float32: torch.full((n,), 7.0, dtype=dt, device=DEV)
    wave, start, length = torch.zeros(1000, device=DEV), torch.zeros(1, dtype=torch.int64, device=DEV), torch.full((1,), 1000, dtype=torch.int64, device=DEV)
    p, s = L.ptr, L.stream_ptr()
    stats, wt, out = sentinel(2), torch.zeros(16 * 10, device=DEV), sentinel(256 * 16)
    gm, gr, blocks = sentinel(16), sentinel(16), torch.tensor([0, 256], dtype=torch.int64, device=DEV)
    calls = [
        (1, L.lib.mts_w2v_wave_stats(s, 0, p(wave), 1000, p(start), p(length), p(stats))),
        (1, L.lib.mts_w2v_wave_stats(s, 1, p(wave), 0, p(start), p(length), p(stats))),
        (1, L.lib.mts_w2v_wave_stats(s, 1, None, 1000, p(start), p(length), p(stats))),
        (2, L.lib.mts_w2v_conv0_stats(s, 1, 12, 10, 5, p(wave), 1000, p(start), p(length), p(stats), p(wt), 1e-5, p(gm), p(gr))),
        (2, L.lib.mts_w2v_conv0_stats(s, 1, 16, 33, 5, p(wave), 1000, p(start), p(length), p(stats), p(wt), 1e-5, p(gm), p(gr))),
        (2, L.lib.mts_w2v_conv0_stats(s, 1, 16, 10, 500, p(wave), 1000, p(start), p(length), p(stats), p(wt), 1e-5, p(gm), p(gr))),
        (1, L.lib.mts_w2v_conv0_stats(s, 1, 16, 10, 5, p(wave), 1000, p(start), p(length), p(stats), p(wt), -1.0, p(gm), p(gr))),
        (1, L.lib.mts_w2v_conv0_stats(s, 1, 16, 10, 5, p(wave), 1000, p(start), p(length), None, p(wt), 1e-5, p(gm), p(gr))),
        (1, L.lib.mts_w2v_conv0(s, 0, 1, 16, 10, 5, p(wave), 1000, p(start), p(length), p(stats), p(wt), p(gm), p(gr), p(gm), p(gr), p(blocks), 200, p(out))),
        (1, L.lib.mts_w2v_conv0(s, 5, 1, 16, 10, 5, p(wave), 1000, p(start), p(length), p(stats), p(wt), p(gm), p(gr), p(gm), p(gr), p(blocks), 256, p(out))),
        (2, L.lib.mts_w2v_conv0(s, 0, 1, 20, 10, 5, p(wave), 1000, p(start), p(length), p(stats), p(wt), p(gm), p(gr), p(gm), p(gr), p(blocks), 256, p(out))),
        (1, L.lib.mts_w2v_conv0(s, 0, 1, 16, 10, 5, p(wave), 1000, p(start), p(length), p(stats), p(wt), p(gm), p(gr), p(gm), p(gr), None, 256, p(out))),
        (2, L.lib.mts_w2v_regroup(s, 0, 1, 128, 4, 15, p(out), p(start), p(blocks), 32, p(out))),
        (2, L.lib.mts_w2v_regroup(s, 0, 1, 128, 4, 130, p(out), p(start), p(blocks), 32, p(out))),
        (2, L.lib.mts_w2v_regroup(s, 0, 1, 48, 4, 16, p(out), p(start), p(blocks), 32, p(out))),
        (1, L.lib.mts_w2v_regroup(s, 3, 1, 128, 4, 16, p(out), p(start), p(blocks), 32, p(out))),
        (1, L.lib.mts_w2v_regroup(s, 0, 1, 128, 4, 16, p(out), p(start), p(blocks), 0, p(out))),
        (1, L.lib.mts_w2v_rows(s, 0, 0, 1, 6, p(wave), p(start), None, None, p(blocks), 4, p(out))),
        (1, L.lib.mts_w2v_rows(s, 0, 0, 1, 8, p(wave), p(start), p(wave), None, p(blocks), 4, p(out))),
        (1, L.lib.mts_w2v_rows(s, 0, 4, 1, 8, p(wave), p(start), None, None, p(blocks), 4, p(out))),
        (1, L.lib.mts_w2v_pos_conv(s, 1, 128, 4, 16, p(wave), p(start), p(blocks), p(blocks), 0, p(wave), p(wave), p(out))),
        (2, L.lib.mts_w2v_pos_conv(s, 1, 1024, 8, 16, p(wave), p(start), p(blocks), p(blocks), 1, p(wave), p(wave), p(out))),
        (2, L.lib.mts_w2v_pos_conv(s, 1, 64, 8, 2, p(wave), p(start), p(blocks), p(blocks), 1, p(wave), p(wave), p(out))),
        (1, L.lib.mts_w2v_pos_conv(s, 1, 128, 4, 16, p(wave), p(start), p(blocks), None, 1, p(wave), p(wave), p(out))),
    ]
    torch.cuda.synchronize()
    assert [got for _, got in calls] == [want for want, _ in calls]
    for t in (stats, out, gm, gr):
        assert bool((t == 7.0).all())
