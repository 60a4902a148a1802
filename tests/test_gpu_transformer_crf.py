"""GPU tests of the Transformer-CRF tagger and of the packed-row CRF entry points under it.

1. mts_crf_nll_packed / mts_crf_viterbi_packed / mts_crf_marginals_packed against the padded entry points, BITWISE: the packed form is the
   same arithmetic at other addresses.  Emissions uniform in +-30 and transitions in +-10 (the range of tests/test_gpu_crf.py); every
   launch is repeated and must give the same bits; a guard region behind the packed outputs must stay untouched.
2. (The LayerNorm backward's head gradients at n_out 3 and 4 are not built: DESIGN.md "Transformer-CRF tagger" has the register numbers.
   The tagger takes the head's parameter gradients from the stored last-layer output, the route every head wider than two outputs takes.)
3. TransformerCRF against the fp64 oracle tests/transformer_crf_oracle.py: loss, every parameter gradient, Viterbi paths, marginal logits;
   packed and padded, fp32 and bf16, restricted and full attention.
4. Through the layers on a resident corpus of 6 documents: NativeTrainer, fit with the threshold search, evaluate, predict, state_dict.
"""
import functools

import numpy as np
import pytest
import torch

from oracle import restatement as R
from tests import transformer_crf_oracle as O

pytestmark = pytest.mark.gpu
DEV = 'cuda'
GUARD, GUARD_VALUE, SENTINEL = 64, 123.25, -77


@pytest.fixture(scope='module')
def ops():
    from multimodaltopicsegmentation_amd import ops as o
    return o


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b, msg):
    assert a.shape == b.shape and torch.equal(_bits(a), _bits(b)), f'{msg}: bits differ'


# ------------------------------------------------------------------------------------------------ 1. packed against padded
def _lengths(B, L, g):
    """0, 1 and L in one batch wherever the batch has room for them; the rest random in 0..L"""
    lengths = torch.randint(0, L + 1, (B,), generator=g).tolist()
    if B == 1:
        return [L]
    lengths[0], lengths[1], lengths[2] = L, 0, 1                       # (every batch but the single document has 16 or more)
    if B > 16:
        lengths[15], lengths[16] = 0, L                                # around the quad kernels' 16-document workgroup
    if B > 64:
        lengths[63], lengths[64] = 1, L                                # around the generic kernels' 64-document workgroup
    return lengths


def _crf_case(B, L, C, seed, lengths=None):
    g = torch.Generator().manual_seed(seed)
    lengths = _lengths(B, L, g) if lengths is None else lengths
    feats = (torch.rand(B, L, C, generator=g) * 2 - 1) * 30
    trans = (torch.rand(C, C, generator=g) * 2 - 1) * 10
    trans[C - 2, :] = R.IMPOSSIBLE
    trans[:, C - 1] = R.IMPOSSIBLE
    tags = torch.zeros(B, L + 3)                                        # Lt > L
    for b, n in enumerate(lengths):
        tags[b, :n] = torch.randint(0, C - 2, (n,), generator=g).float()
    row0 = np.zeros(B, dtype=np.int64)
    row0[1:] = np.cumsum(lengths[:-1])
    n_rows = int(sum(lengths))
    packed = torch.cat([feats[b, :n] for b, n in enumerate(lengths)] + [feats.new_zeros(0, C)]).contiguous()
    return dict(B=B, L=L, C=C, lengths=lengths, feats=feats.to(DEV), trans=trans.to(DEV), tags=tags.to(DEV), row0=row0.tolist(),
                n_rows=n_rows, packed=packed.to(DEV), li32=torch.tensor(lengths, dtype=torch.int32, device=DEV),
                row0_d=torch.tensor(row0, dtype=torch.int32, device=DEV))


def _guarded(n, dtype=torch.float32):
    """n elements to be written (pre-filled with NaN) + GUARD elements that must stay as they are"""
    buf = torch.full((n + GUARD,), GUARD_VALUE, dtype=dtype, device=DEV)
    buf[:n] = float('nan')
    return buf


def _guard_intact(buf, n, msg):
    assert bool((buf[n:] == GUARD_VALUE).all()), f'{msg}: the guard region behind the output was written'


def _padded_runs(ops, c):
    B, L, C = c['B'], c['L'], c['C']
    out = torch.full((2,), float('nan'), device=DEV)
    df = torch.full((B, L, C), float('nan'), device=DEV)
    dt = torch.full((C, C), float('nan'), device=DEV)
    ops.crf_nll(c['feats'], c['tags'], c['li32'], c['trans'], out, df, dt)
    score = torch.full((B,), float('nan'), device=DEV)
    paths = torch.full((B, L), SENTINEL, dtype=torch.int32, device=DEV)
    ops.crf_viterbi(c['feats'], c['li32'], c['trans'], score, paths)
    sc = torch.full((B, L), float('nan'), device=DEV)
    logz = torch.full((B,), float('nan'), device=DEV)
    ops.crf_marginals(c['feats'], c['li32'], c['trans'], sc, cls=1, logz=logz)
    return dict(loss=out[:1].cpu(), df=df.cpu(), dt=dt.cpu(), score=score.cpu(), paths=paths.cpu(), sc=sc.cpu(), logz=logz.cpu())


def _packed_runs(ops, c, packed=True):
    """packed=False: the packed entry points with row0 = NULL on the padded buffers"""
    B, L, C = c['B'], c['L'], c['C']
    feats = c['packed'] if packed else c['feats'].view(B * L, C)
    row0 = c['row0_d'] if packed else None
    n = feats.shape[0]
    out = torch.full((2,), float('nan'), device=DEV)
    df = _guarded(n * C)
    dt = torch.full((C, C), float('nan'), device=DEV)
    ops.crf_nll_packed(feats, c['tags'], c['li32'], c['trans'], out, (B, L), row0=row0, dfeats=df[:n * C].view(n, C), dtrans=dt)
    _guard_intact(df, n * C, 'dfeats')
    score = torch.full((B,), float('nan'), device=DEV)
    paths = torch.full((B, L), SENTINEL, dtype=torch.int32, device=DEV)
    ops.crf_viterbi_packed(feats, c['li32'], c['trans'], score, paths, row0=row0)
    sc = _guarded(n)
    logz = torch.full((B,), float('nan'), device=DEV)
    ops.crf_marginals_packed(feats, c['li32'], c['trans'], sc[:n], (B, L), row0=row0, cls=1, logz=logz)
    _guard_intact(sc, n, 'scores')
    return dict(loss=out[:1].cpu(), df=df[:n * C].view(n, C).cpu(), dt=dt.cpu(), score=score.cpu(), paths=paths.cpu(), sc=sc[:n].cpu(),
                logz=logz.cpu())


def _check_packed_equals_padded(ops, c):
    pad = _padded_runs(ops, c)
    pk = _packed_runs(ops, c)
    again = _packed_runs(ops, c)
    for k in pk:
        assert torch.equal(_bits(pk[k]), _bits(again[k])), f'{k}: the second launch gave other bits'
    null = _packed_runs(ops, c, packed=False)
    B, L, C = c['B'], c['L'], c['C']
    for k in ('loss', 'dt', 'score', 'logz'):
        _same_bits(pk[k], pad[k], f'packed {k}')
        _same_bits(null[k], pad[k], f'row0 = NULL {k}')
    assert torch.equal(pk['paths'], pad['paths']) and torch.equal(null['paths'], pad['paths'])
    _same_bits(null['df'].view(B, L, C), pad['df'], 'row0 = NULL dfeats')
    _same_bits(null['sc'].view(B, L), pad['sc'], 'row0 = NULL scores')
    assert not torch.isnan(pk['df']).any() and not torch.isnan(pk['sc']).any(), 'a packed row was left unwritten'
    for b, n in enumerate(c['lengths']):
        r = c['row0'][b]
        _same_bits(pk['df'][r:r + n], pad['df'][b, :n], f'dfeats of document {b}')
        _same_bits(pk['sc'][r:r + n], pad['sc'][b, :n], f'scores of document {b}')
        assert bool((pad['paths'][b, n:] == -1).all())
    return pad, pk


@pytest.mark.parametrize('L', [1, 7, 300])
@pytest.mark.parametrize('B', [1, 16, 17, 33])
def test_packed_equals_padded_c4(ops, B, L):
    """The quad kernels (16 documents per workgroup): one full workgroup, one document more, and three workgroups with a partial last."""
    _check_packed_equals_padded(ops, _crf_case(B, L, 4, 100 * B + L))


@pytest.mark.parametrize('L', [1, 7, 300])
@pytest.mark.parametrize('B', [1, 64, 65])
@pytest.mark.parametrize('C', [3, 5])
def test_packed_equals_padded_generic(ops, C, B, L):
    """The generic kernels (one thread per document, 64 per workgroup)."""
    _check_packed_equals_padded(ops, _crf_case(B, L, C, 1000 * C + 10 * B + L))


def test_packed_viterbi_beyond_the_lds_opt_in(ops):
    """A 10 241-sentence document next to a 3-sentence one: C == 4 leaves the LDS back-pointers for the generic kernel, whose back-pointer
    workspace is [n_rows, C] in the packed form.  Paths and scores bitwise the padded call's (which tests/test_gpu_crf.py holds to the
    oracle at this length)."""
    L = 10241
    c = _crf_case(2, L, 4, 3004, lengths=[L, 3])
    want_s = torch.full((2,), float('nan'), device=DEV)
    want_p = torch.full((2, L), SENTINEL, dtype=torch.int32, device=DEV)
    ops.crf_viterbi(c['feats'], c['li32'], c['trans'], want_s, want_p)
    for _ in range(2):
        score = torch.full((2,), float('nan'), device=DEV)
        paths = torch.full((2, L), SENTINEL, dtype=torch.int32, device=DEV)
        ops.crf_viterbi_packed(c['packed'], c['li32'], c['trans'], score, paths, row0=c['row0_d'])
        _same_bits(score.cpu(), want_s.cpu(), 'viterbi score')
        assert torch.equal(paths.cpu(), want_p.cpu())
    assert bool((want_p[1, 3:] == -1).all()) and bool((want_p[0] >= 0).all())


@pytest.mark.parametrize('C', [4, 5])
def test_packed_document_out_of_range_contributes_nothing(ops, C):
    """row0 entries that would put a document's rows outside [0, n_rows) -- negative, and one row too far -- form no address: the other
    documents' results keep their bits, the document adds nothing to the loss sum (B still divides) and writes no row."""
    B, L = 5, 9
    c = _crf_case(B, L, C, 7000 + C, lengths=[9, 4, 1, 6, 3])
    good = _packed_runs(ops, c)
    n = c['n_rows']
    bad_row0 = list(c['row0'])
    bad_row0[1] = -1                                                  # rows -1 .. 2
    bad_row0[4] = n - 3 + 1                                           # its last row would be row n_rows
    c2 = dict(c, row0_d=torch.tensor(bad_row0, dtype=torch.int32, device=DEV))
    got = _packed_runs(ops, c2)
    per_doc = []
    for b in range(B):                                                # each document's own loss term: a batch of one
        one = _crf_case(1, L, C, 0, lengths=[c['lengths'][b]])
        one.update(feats=c['feats'][b:b + 1].contiguous(), tags=c['tags'][b:b + 1].contiguous(), trans=c['trans'])
        per_doc.append(float(_padded_runs(ops, one)['loss']))
    want = (per_doc[0] + per_doc[2] + per_doc[3]) / B
    assert abs(float(got['loss']) - want) < 1e-5 * max(1.0, abs(want)), (float(got['loss']), want)
    assert abs(float(good['loss']) - sum(per_doc) / B) < 1e-5 * max(1.0, abs(sum(per_doc) / B))
    for b in (0, 2, 3):
        r, k = c['row0'][b], c['lengths'][b]
        _same_bits(got['df'][r:r + k], good['df'][r:r + k], f'dfeats of document {b}')
        _same_bits(got['sc'][r:r + k], good['sc'][r:r + k], f'scores of document {b}')
        _same_bits(got['score'][b:b + 1], good['score'][b:b + 1], f'viterbi score of document {b}')
        _same_bits(got['logz'][b:b + 1], good['logz'][b:b + 1], f'log Z of document {b}')
        assert torch.equal(got['paths'][b], good['paths'][b])
    for b in (1, 4):
        r, k = c['row0'][b], c['lengths'][b]
        assert bool(torch.isnan(got['df'][r:r + k]).all()) and bool(torch.isnan(got['sc'][r:r + k]).all())      # (NaN / B is a NaN)
        assert float(got['score'][b]) == 0.0 and float(got['logz'][b]) == 0.0 and bool((got['paths'][b] == -1).all())


# ------------------------------------------------------------------------------------------------ 3. the tagger against the oracle
D, FF, HEADS, WINDOW = 64, 32, 2, 6            # window 6: the last layer's one-sided radius is 3 (every pyramidal window must be even)
LENGTHS = [40, 1, 2, 9, 33]                    # the encoder's own tests go down to one sentence, not to none
# chosen on the CPU: the oracle's recursion in fp32 decodes the fp64 oracle's paths, and so it does on emissions moved by 5e-2 (asserted)
SEEDS = {(1, True): 8, (2, True): 8, (1, False): 8}


def _tagger(num_layers, restricted, dtype, decode='viterbi', seed=None):
    from multimodaltopicsegmentation_amd import TransformerCRF
    seed = SEEDS[(num_layers, restricted)] if seed is None else seed
    return TransformerCRF(2, D, FF, num_layers=num_layers, nheads=HEADS, window_size=WINDOW, restricted=restricted, decode=decode,
                          compute_dtype=dtype, max_position_embedding=128, seed=seed)


def _inputs(seed):
    g = torch.Generator().manual_seed(1000 + seed)
    B, L = len(LENGTHS), max(LENGTHS)
    x = torch.randn(B, L, D, generator=g)
    y = torch.zeros(B, L)
    for b, n in enumerate(LENGTHS):
        x[b, n:] = 0.0
        y[b, :n] = (torch.rand(n, generator=g) < 0.3).float()
    return x, y, torch.tensor(LENGTHS)


@functools.lru_cache(maxsize=None)
def _reference(num_layers, restricted):
    """The fp64 oracle of one configuration, computed once: loss, gradients, emissions, Viterbi, marginal logits."""
    m = _tagger(num_layers, restricted, 'fp32')
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    p = {k: v.double().requires_grad_(True) for k, v in sd.items()}
    x, y, lens = _inputs(SEEDS[(num_layers, restricted)])
    h = O.encode(x.double(), lens, p, HEADS, num_layers, WINDOW, restricted)
    loss = O.loss(h, lens, y.double(), p)
    loss.backward()
    with torch.no_grad():
        pd = {k: v.detach() for k, v in p.items()}
        hd = h.detach()
        score, paths = O.viterbi(hd, lens, pd)
        score32, paths32 = O.viterbi(hd.float(), lens, {k: v.float() for k, v in pd.items()})
        em = O.emissions(hd, pd)
        g = torch.Generator().manual_seed(9)
        moved = em + (torch.rand(em.shape, generator=g, dtype=torch.float64) * 2 - 1) * 5e-2
        _, paths_moved = R.crf_viterbi(moved, R.create_mask(em.shape[1], lens), torch.eye(4, dtype=torch.float64), torch.zeros(4, dtype=torch.float64),
                                       pd['crf.transitions'])
        logit = O.marginal_logits(hd, lens, pd)
    return dict(sd=sd, grads={k: v.grad for k, v in p.items()}, loss=float(loss.detach()), score=score, paths=paths, paths32=paths32, score32=score32,
                paths_moved=paths_moved, em=em, logit=logit, trans=pd['crf.transitions'], x=x, y=y, lens=lens)


def test_the_seeds_pose_the_path_comparison_well():
    """A property of the inputs, checked without the GPU: at the chosen seeds no Viterbi decision of the fp64 oracle lies inside fp32
    rounding (the oracle's own recursion in fp32 finds the same paths) nor inside the bf16 emission bound of tests/test_gpu_taggers.py."""
    for (nl, restricted) in SEEDS:
        ref = _reference(nl, restricted)
        assert ref['paths32'] == ref['paths'], (nl, restricted)
        assert ref['paths_moved'] == ref['paths'], (nl, restricted)
        assert [len(p_) for p_ in ref['paths']] == LENGTHS
        assert len({t for p_ in ref['paths'] for t in p_}) == 2, 'the paths use one tag only: nothing to compare'


def _check_grads(m, ref, f32, packed):
    grads = m.grad_views()
    worst = []
    for n in grads:
        r = ref['grads'][n]
        if r is None or 'key.bias' in n:          # (the key bias shifts every score of a softmax row alike: its gradient is rounding noise)
            continue
        a = m.logical_view(grads, n).detach().cpu().double()
        assert a.shape == r.shape, n
        scale = max(float(r.abs().max()), 1e-8)
        if n.startswith('crf.'):                  # the head: tests/test_gpu_crf.py::test_crf_model_with_a_single_tag
            lim = (3e-3 if f32 else 0.15) * scale + (2e-7 if f32 else 3e-4)
        else:                                     # the encoder: tests/test_gpu_taggers.py::test_default_hidden_size_25_transformer
            lim = (3e-3 if f32 else 0.12) * scale + (2e-7 if f32 else 3e-4)
        if 'position_embeddings' in n:
            off = 2 if m.restricted else 0
            assert float(a[max(LENGTHS) + off:].abs().max()) == 0.0
        worst.append((float((a - r).abs().max()) / lim, n))
    print(f'packed={packed}: worst gradient error / limit {max(worst)[0]:.3f} at {max(worst)[1]}')
    assert max(worst)[0] < 1.0, sorted(worst)[-3:]
    assert {'crf.fc.weight', 'crf.fc.bias', 'crf.transitions'} <= {n for _, n in worst}


@pytest.mark.parametrize('dtype', ['fp32', 'bf16'])
@pytest.mark.parametrize('num_layers,restricted', [(1, True), (2, True), (1, False)])
def test_tagger_against_the_oracle(num_layers, restricted, dtype):
    """Loss and every parameter gradient, packed and padded, against the fp64 oracle and against each other (the bounds of
    tests/test_gpu_taggers.py::test_packed_batch_gives_the_same_loss_and_gradients); emissions to the logit bounds of test_gpu_taggers.py;
    Viterbi paths exactly in fp32, by the bf16 rule of tests/test_gpu_parity_fullsize.py otherwise; the marginal logits within the kernel's
    own 2e-3 (tests/test_gpu_crf_marginal.py) plus what the emission bound e can move a logit of an n-sentence document, 2 n e (the
    logit's derivative by an emission row is a difference of two conditional distributions)."""
    ref = _reference(num_layers, restricted)
    f32 = dtype == 'fp32'
    m = _tagger(num_layers, restricted, dtype)
    m.load_state_dict(ref['sd'])
    m = m.to(DEV).eval()                                               # eval: the full-attention form trains with attention dropout 0.1
    x, y, lens = ref['x'].to(DEV), ref['y'].to(DEV), ref['lens']
    flat = {}
    for packed in (False, True):
        m.pack_rows = packed
        loss, feats = m.loss_and_grad(x, lens, y, True)
        assert feats.shape == ((sum(LENGTHS), 4) if packed else (len(LENGTHS), max(LENGTHS), 4))
        print(f'{dtype} packed={packed}: loss {loss.item():.7f}, oracle {ref["loss"]:.7f}')
        assert abs(loss.item() - ref['loss']) < (5e-6 if f32 else 3e-2) * max(1.0, abs(ref['loss']))
        _check_grads(m, ref, f32, packed)
        flat[packed] = (loss.item(), m.grad_flat().clone())
        em = feats.float().cpu().double()
        r = 0
        for b, n in enumerate(LENGTHS):
            got = em[r:r + n] if packed else em[b, :n]
            r += n
            assert float((got - ref['em'][b, :n]).abs().max()) < (3e-5 if f32 else 5e-2), (packed, b)
        loss_only = m.loss_and_grad(x, lens, y, False)[0]
        assert loss_only.item() == loss.item()
    assert abs(flat[True][0] - flat[False][0]) < (1e-6 if f32 else 2e-3) * max(1.0, abs(flat[False][0]))
    scale = float(flat[False][1].abs().max())
    assert float((flat[True][1] - flat[False][1]).abs().max()) < (2e-5 if f32 else 2e-2) * scale
    # Viterbi
    score, paths = m(x, lens)
    assert [len(p_) for p_ in paths] == LENGTHS and tuple(score.shape) == (len(LENGTHS),)
    if f32:
        assert paths == ref['paths']
        np.testing.assert_allclose(score.cpu().numpy(), ref['score'].numpy(), rtol=1e-5, atol=1e-4)
    else:
        agree = 0
        for b, n in enumerate(LENGTHS):
            best = float(ref['score'][b])
            here = float(O.path_score(ref['em'][b, :n], paths[b], ref['trans']))
            assert here <= best + 1e-3 and best - here < 2e-2 * max(1.0, abs(best)), b
            agree += sum(int(a == r_) for a, r_ in zip(paths[b], ref['paths'][b]))
        assert agree >= 0.97 * sum(LENGTHS), (agree, sum(LENGTHS))
    # marginal logits
    mm = _tagger(num_layers, restricted, dtype, decode='marginal')
    mm.load_state_dict(ref['sd'])
    mm = mm.to(DEV).eval()
    scores, tags = mm(x, lens, 0.5)
    assert scores.shape == (len(LENGTHS), max(LENGTHS), 1) and torch.equal(scores, m.marginal_scores(x, lens))
    s = scores.cpu().view(len(LENGTHS), -1).double()
    e = 3e-5 if f32 else 5e-2
    for b, n in enumerate(LENGTHS):
        err = float((s[b, :n] - ref['logit'][b, :n]).abs().max())
        assert err < 2e-3 + 2 * n * e, (b, err)
        assert bool((s[b, n:] == 0).all())
        prob = torch.sigmoid(ref['logit'][b, :n])
        if f32:
            assert all(tags[b][i] == bool(prob[i] > 0.5) for i in range(n) if abs(float(prob[i]) - 0.5) > 1e-3)
    assert [len(t) for t in tags] == LENGTHS


# ------------------------------------------------------------------------------------------------ 4. through the layers
DOC_LENGTHS = [21, 5, 40, 8, 13, 35]


def _docs(seed=2):
    from tests.test_gpu_fit import _corpus
    return _corpus('transformer', DOC_LENGTHS, seed)


def _small(decode='viterbi', seed=11):
    from multimodaltopicsegmentation_amd import TransformerCRF
    return TransformerCRF(2, 64, 32, num_layers=2, nheads=4, window_size=4, decode=decode, compute_dtype='fp32', max_position_embedding=128,
                          seed=seed).to(DEV)


@pytest.mark.parametrize('kw', [dict(optimizer='Adam'), dict(optimizer='SGD', lr=1e-2), dict(optimizer='Adam', gradient_clip_val=0.5)],
                         ids=['adam', 'sgd', 'adam-clipped'])
def test_native_trainer_lowers_the_loss(kw):
    from multimodaltopicsegmentation_amd.trainer import NativeTrainer
    corpus = _docs()
    model = _small()
    tr = NativeTrainer(model, **{'lr': 1e-3, **kw})
    batch = corpus.batch(list(range(len(corpus))))
    losses = [float(tr.step(batch)) for _ in range(20)]
    print(kw, 'first', losses[0], 'last', losses[-1])
    assert all(np.isfinite(losses)) and losses[-1] < losses[0]
    if kw.get('gradient_clip_val'):
        assert float(tr.last_grad_norm) > 0 and 0 < float(tr.last_clip_coef) <= 1.0


def test_text_segmenter_steps_through_autograd():
    """The Lightning-style path: training_step returns a loss wired into autograd through the one native node, .backward() hands every
    parameter the native gradient, a torch optimizer moves the parameters, validation_step returns the loss without gradients."""
    from multimodaltopicsegmentation_amd import TextSegmenter
    torch.manual_seed(3)
    corpus = _docs()
    batch = corpus.batch(list(range(len(corpus))))
    ts = TextSegmenter(2, 64, 32, num_layers=2, architecture='Transformer-CRF', nheads=4, attention_window=4, compute_dtype='fp32', lr=1e-3,
                       optimizer='SGD').to(DEV)
    opt = ts.configure_optimizers()['optimizer']
    loss = ts.training_step(batch, 0)
    assert loss.requires_grad and loss.dim() == 0
    loss.backward()
    native = {n: v.detach().clone() for n, v in ts.model.grad_views().items()}
    params = dict(ts.model.named_parameters())
    assert set(params) == set(native) and {'crf.fc.weight', 'crf.fc.bias', 'crf.transitions'} <= set(params)
    for n, prm in params.items():
        assert prm.grad is not None and torch.equal(prm.grad, native[n]), n
    assert float(params['crf.transitions'].grad.abs().max()) > 0 and float(params['crf.fc.weight'].grad.abs().max()) > 0
    before = ts.model.flat.detach().clone()
    val = ts.validation_step(batch, 0)
    assert not val.requires_grad and val.item() == loss.item()
    opt.step()
    assert not torch.equal(ts.model.flat, before)
    assert ts.validation_step(batch, 0).item() < loss.item()
    tags = ts.predict_step(batch, 0)
    assert [len(t) for t in tags] == DOC_LENGTHS and {v for t in tags for v in t} <= {0, 1}


def test_fit_searches_a_threshold_with_the_marginal_decode():
    from multimodaltopicsegmentation_amd.trainer import NativeTrainer
    model = _small(decode='marginal')
    out = NativeTrainer(model, lr=1e-3).fit(_docs(2), _docs(6), batch_size=4, max_epochs=2, seed=5, search_threshold=True, metric='Pk')
    assert out['threshold'] is not None and model.th == out['threshold'] and 0 < out['threshold'] < 1
    assert len(out['epochs']) == 2 and all(np.isfinite(r['monitored']) for r in out['epochs'])
    with pytest.raises(NotImplementedError, match="'Transformer-CRF' decodes by Viterbi"):
        NativeTrainer(_small(), lr=1e-3).fit(_docs(2), _docs(6), batch_size=4, max_epochs=1, search_threshold=True, metric='Pk')


def test_evaluate_equals_test_step_with_the_viterbi_decode():
    from multimodaltopicsegmentation_amd import TextSegmenter, evaluate
    torch.manual_seed(3)
    test = _docs(8)
    ts = TextSegmenter(2, 64, 32, num_layers=2, architecture='Transformer-CRF', nheads=4, attention_window=4, compute_dtype='fp32',
                       metric='Pk').to(DEV).eval()
    res = ts.test_step(test.batch(list(range(len(test)))), 0)
    ev = evaluate(ts, test, batch_size=len(test))
    print('test_step', res, 'evaluate', ev['mean'])
    assert (ev['mean']['Pk'], ev['mean']['WD'], ev['mean']['F1']) == (res['test_loss'], res['WD_loss'], res['F1_loss'])
    assert ev['threshold'] == 0.5
    with pytest.raises(ValueError, match='min_segment > 1 needs probabilities'):
        evaluate(ts, test, min_segment=2)


def test_predict_min_segment_with_the_marginal_decode():
    from multimodaltopicsegmentation_amd import predict
    corpus = _docs(8)
    model = _small(decode='marginal').eval()
    p = np.concatenate(predict(model, corpus, batch_size=4, threshold=0.5, return_probabilities=True).probabilities)
    th = float(np.median(p))                                            # half of the sentences are boundaries before the constraint
    free = predict(model, corpus, batch_size=4, threshold=th, return_tags=True)
    pred = predict(model, corpus, batch_size=4, threshold=th, min_segment=2, return_tags=True)
    assert pred.min_segment == 2 and pred.threshold == th
    sizes_free = np.concatenate([np.diff(np.concatenate([[0], e])) for e in free.segment_ends])
    assert int(sizes_free.min()) == 1, 'the unconstrained decode has no one-sentence segment: the constraint is not exercised'
    for d, n in enumerate(DOC_LENGTHS):                                 # (the bound of tests/test_gpu_predict.py)
        assert np.diff(np.concatenate([[0], pred.segment_ends[d]])).min() >= min(2, n), d
        assert int(pred.segment_ends[d][-1]) == n
    assert sum(int(t.sum()) for t in pred.tags) < sum(int(t.sum()) for t in free.tags)
    with pytest.raises(ValueError, match='min_segment > 1 needs probabilities'):
        predict(_small().eval(), corpus, min_segment=2)


def test_state_dict_round_trip_reproduces_the_scores():
    corpus = _docs(8)
    batch = corpus.batch(list(range(len(corpus))))
    a = _small(decode='marginal', seed=11).eval()
    b = _small(decode='marginal', seed=12).eval()
    sa = a(batch['src_tokens'], batch['src_lengths'])[0]
    assert not torch.equal(sa, b(batch['src_tokens'], batch['src_lengths'])[0])
    sd = {k: v.detach().cpu().clone() for k, v in a.state_dict().items()}
    b.load_state_dict(sd)
    assert torch.equal(_bits(b(batch['src_tokens'], batch['src_lengths'])[0]), _bits(sa))
    va, vb = _small(seed=11).eval(), _small(seed=12).eval()
    vb.load_state_dict(sd)
    (s1, p1), (s2, p2) = va(batch['src_tokens'], batch['src_lengths']), vb(batch['src_tokens'], batch['src_lengths'])
    assert torch.equal(_bits(s1), _bits(s2)) and p1 == p2
