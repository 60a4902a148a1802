"""The CRF kernels of csrc/crf.hip beyond the one path the other GPU tests run (C == 4, Gaussian inputs, every operand given): the generic
kernels for C in 3..8 (log-domain alpha / beta sweeps, 64 documents per block, int32 back-pointers in global memory, crf_finish_kernel
over C * C + 1 partial sums), first-max tie breaking, the C == 4 Viterbi fallback beyond the LDS opt-in, optional operands, documents
of length 0, the numeric range of the scaled-probability recursion, and a C == 3 model.

The reference is oracle.restatement in fp64: crf_forward_score - crf_gold_score, .mean(), autograd for both gradients, crf_viterbi
with an identity fc.  Every transition table has row START and column STOP at IMPOSSIBLE, as the models build it.  dfeats is pre-filled
with NaN and paths with a sentinel: rows past a document's length must come back exactly 0 / exactly -1.  Every launch is repeated once
and must give the same bits.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import restatement as R  # noqa: E402


@pytest.fixture(scope='module')
def ops():
    from multimodaltopicsegmentation_amd import ops as o
    return o


DEV = 'cuda'
SENTINEL = -77

# tolerances of tests/test_gpu_kernels.py::test_crf_nll_viterbi
TOL_LOSS = 1e-4
TOL_DF = dict(rtol=1e-3, atol=1e-6)
TOL_DT = dict(rtol=1e-3, atol=1e-5)
TOL_SCORE = dict(rtol=1e-5, atol=1e-4)


def _close(got, ref, rtol, atol, msg=''):
    got = got.detach().float().cpu().double()
    ref = ref.detach().double()
    err = (got - ref).abs()
    lim = atol + rtol * ref.abs()
    bad = err > lim
    print(f'{msg}: max err {float(err.max()):.3e}, worst err / limit {float((err / lim).max()):.3f} (ref max {float(ref.abs().max()):.3e})')
    assert not bad.any(), f'{msg}: {int(bad.sum())}/{bad.numel()} off, max err {float(err.max()):.3e} (ref max {float(ref.abs().max()):.3e})'


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b, msg):
    assert a.shape == b.shape and torch.equal(_bits(a), _bits(b)), f'{msg}: bits differ'


def _mask_table(trans):
    C = trans.shape[0]
    trans[C - 2, :] = R.IMPOSSIBLE
    trans[:, C - 1] = R.IMPOSSIBLE
    return trans


def _gold_tags(B, width, C, lengths, g):
    """Gold tags from the real tags 0..C-3 inside each length, 0 past it."""
    tags = torch.zeros(B, width)
    for b, n in enumerate(lengths):
        tags[b, :n] = torch.randint(0, C - 2, (n,), generator=g).float()
    return tags


def _oracle_nll(feats, tags, lengths, trans, dtype=torch.float64):
    """(loss, dfeats, dtrans) of mean(logZ - gold) by autograd, in `dtype` on the CPU."""
    L = feats.shape[1]
    f = feats.to(dtype).requires_grad_(True)
    t = trans.to(dtype).requires_grad_(True)
    mask = R.create_mask(L, torch.as_tensor(lengths)).to(dtype)
    per_doc = R.crf_forward_score(f, mask, t) - R.crf_gold_score(f, tags[:, :L].long(), mask, t)
    loss = per_doc.mean()
    loss.backward()
    return loss.detach(), f.grad, t.grad, per_doc.detach()


def _oracle_viterbi(feats, lengths, trans):
    C = feats.shape[2]
    mask = R.create_mask(feats.shape[1], torch.as_tensor(lengths)).double()
    return R.crf_viterbi(feats.double(), mask, torch.eye(C, dtype=torch.float64), torch.zeros(C, dtype=torch.float64), trans.double())


def _run_nll(ops, feats, tags, lengths, trans, want_df=True, want_dt=True):
    """Two launches on fresh NaN-filled outputs, the same bits required; -> (loss, dfeats, dtrans) on the CPU."""
    B, L, C = feats.shape
    fd, td, trd = feats.to(DEV), tags.to(DEV), trans.to(DEV)
    li32 = None if lengths is None else torch.as_tensor(lengths, dtype=torch.int32).to(DEV)
    runs = []
    for _ in range(2):
        out = torch.full((2,), float('nan'), device=DEV)
        df = torch.full((B, L, C), float('nan'), device=DEV) if want_df else None
        dt = torch.full((C, C), float('nan'), device=DEV) if want_dt else None
        ops.crf_nll(fd, td, li32, trd, out, df, dt)
        runs.append((out[:1].cpu(), None if df is None else df.cpu(), None if dt is None else dt.cpu()))
    for a, b, name in zip(runs[0], runs[1], ('loss', 'dfeats', 'dtrans')):
        if a is not None:
            _same_bits(a, b, f'{name}, second launch')
    loss, df, dt = runs[0]
    if df is not None:
        assert not torch.isnan(df).any(), 'dfeats keeps a NaN of the pre-fill'
        for b, n in enumerate([L] * B if lengths is None else lengths):
            assert bool((df[b, n:] == 0).all()), f'dfeats of document {b} is not exactly 0 past its length {n}'
    return loss, df, dt


def _run_viterbi(ops, feats, lengths, trans):
    """Two launches on sentinel-filled paths, the same bits required; -> (score [B], paths [B, L]) on the CPU."""
    B, L, C = feats.shape
    fd, trd = feats.to(DEV), trans.to(DEV)
    li32 = None if lengths is None else torch.as_tensor(lengths, dtype=torch.int32).to(DEV)
    runs = []
    for _ in range(2):
        score = torch.full((B,), float('nan'), device=DEV)
        paths = torch.full((B, L), SENTINEL, dtype=torch.int32, device=DEV)
        ops.crf_viterbi(fd, li32, trd, score, paths)
        runs.append((score.cpu(), paths.cpu()))
    _same_bits(runs[0][0], runs[1][0], 'viterbi score, second launch')
    assert torch.equal(runs[0][1], runs[1][1]), 'paths, second launch'
    score, paths = runs[0]
    for b, n in enumerate([L] * B if lengths is None else lengths):
        assert bool((paths[b, n:] == -1).all()), f'paths of document {b} are not -1 past its length {n}'
    return score, paths


def _paths_list(paths, lengths):
    return [paths[b, :n].tolist() for b, n in enumerate(lengths)]


def _check_all(ops, feats, tags, lengths, trans):
    """Loss, both gradients, Viterbi score and every path against the fp64 oracle."""
    ref_loss, ref_df, ref_dt, per_doc = _oracle_nll(feats, tags, lengths, trans)
    for b, n in enumerate(lengths):
        if n == 0:
            assert float(per_doc[b]) == 0.0                           # an empty document adds nothing to the loss sum
    loss, df, dt = _run_nll(ops, feats, tags, lengths, trans)
    print(f'loss {float(loss):.9g}, oracle {float(ref_loss):.9g}')
    assert abs(float(loss) - float(ref_loss)) < TOL_LOSS, (float(loss), float(ref_loss))
    _close(df, ref_df, msg='dfeats', **TOL_DF)
    _close(dt, ref_dt, msg='dtrans', **TOL_DT)
    score, paths = _run_viterbi(ops, feats, lengths, trans)
    rs, rp = _oracle_viterbi(feats, lengths, trans)
    _close(score, rs, msg='viterbi score', **TOL_SCORE)
    assert _paths_list(paths, lengths) == rp
    return loss, df, dt, score, paths


# ------------------------------------------------------------------------------------------------ 1. generic C
@pytest.mark.parametrize('B', [1, 17, 65])
@pytest.mark.parametrize('C', [3, 4, 5, 8])
def test_crf_generic_tagset_sizes(ops, C, B):
    """crf_nll_kernel / crf_viterbi_kernel (C = 3, 5, 8) with C = 4 (the quad kernels) as the control: B = 17 crosses the quad kernels'
    16-document block, B = 65 the generic kernels' 64-document block; lengths L, 1, 0 and random ones.  The oracle's loss term of an empty
    document is exactly 0.0 and its path is [].  (The first run of C = 3 found crf_nll_kernel's marginals 3e-5 off an exact 1: DESIGN.md, CRF.)"""
    L = 33
    g = torch.Generator().manual_seed(1000 + 10 * C + B)
    if B == 1:
        length_sets = [[L], [1], [0]]
    else:
        lengths = torch.randint(0, L + 1, (B,), generator=g).tolist()
        lengths[0], lengths[1], lengths[2], lengths[B - 1] = L, 1, 0, L - 2
        if B > 64:
            lengths[63], lengths[64] = 0, L                          # the last document of the first block and the first of the second
        length_sets = [lengths]
    for lengths in length_sets:
        feats = torch.randn(B, L, C, generator=g)
        trans = _mask_table(torch.randn(C, C, generator=g))
        tags = _gold_tags(B, L, C, lengths, g)
        _check_all(ops, feats, tags, lengths, trans)


# ------------------------------------------------------------------------------------------------ 2. ties
def _viterbi_last_max(feats, lengths, trans):
    """oracle.restatement.crf_viterbi with an identity fc, except that every maximum takes the LAST of equal candidates."""
    B, L, C = feats.shape
    start, stop = C - 2, C - 1
    m = R.create_mask(L, torch.as_tensor(lengths)).to(feats.dtype)

    def last_max(v):
        val, idx = v.flip(-1).max(dim=-1)
        return val, v.shape[-1] - 1 - idx

    bps = torch.zeros(B, L, C, dtype=torch.long)
    best = feats.new_full((B, C), R.IMPOSSIBLE)
    best[:, start] = 0
    for t in range(L):
        acc, bps[:, t] = last_max(best.unsqueeze(1) + trans)
        acc = acc + feats[:, t]
        mt = m[:, t].unsqueeze(1)
        best = acc * mt + best * (1 - mt)
    score, tag = last_max(best + trans[stop])
    paths = []
    for b in range(B):
        cur = int(tag[b])
        path = [cur]
        for t in range(int(lengths[b]) - 1, -1, -1):
            cur = int(bps[b, t, cur])
            path.append(cur)
        paths.append(path[-2::-1])
    return score, paths


def _tie_case(C):
    B, L = 24, 40
    g = torch.Generator().manual_seed(2000 + C)
    lengths = torch.randint(L // 2, L + 1, (B,), generator=g).tolist()
    lengths[0] = L
    feats = torch.randint(-2, 3, (B, L, C), generator=g).float()
    trans = _mask_table(torch.randint(-1, 2, (C, C), generator=g).float())
    return feats, lengths, trans


@pytest.mark.parametrize('C', [4, 5, 8])
def test_crf_viterbi_breaks_ties_as_torch_max(ops, C):
    """Integer emissions in [-2, 2] and transitions in [-1, 1]: every sum is exact in fp32 and in fp64, so the score must EQUAL the
    oracle's and every path must be the oracle's, whose torch.max takes the first of equal candidates.  The inputs do tie: a last-max copy
    of the oracle's recursion has to disagree with the oracle on at least half of the documents, or the test fails."""
    feats, lengths, trans = _tie_case(C)
    rs, rp = _oracle_viterbi(feats, lengths, trans)
    ls, lp = _viterbi_last_max(feats.double(), lengths, trans.double())
    differ = sum(a != b for a, b in zip(rp, lp))
    print(f'C = {C}: the last-max recursion differs from the oracle on {differ} of {len(rp)} documents')
    assert torch.equal(ls, rs)                                        # equally good paths: only the choice among them differs
    assert 2 * differ >= len(rp), f'the inputs lost their ties: only {differ} of {len(rp)} documents depend on the tie break'
    score, paths = _run_viterbi(ops, feats, lengths, trans)
    assert torch.equal(score.double(), rs)
    assert _paths_list(paths, lengths) == rp


# ------------------------------------------------------------------------------------------------ 3. the C == 4 Viterbi fallback
@pytest.mark.parametrize('L', [10240, 10241])
def test_crf_viterbi_c4_beyond_the_lds_opt_in(ops, L):
    """16 * L bytes of packed back-pointers fit the 160-KiB LDS opt-in up to L = 10 240 (crf_viterbi4_kernel); one step more and C == 4
    runs the generic kernel with its int32 back-pointers in global memory.  Every tag and the score against the oracle, tolerances of
    test_crf_long_documents.

    The seed is one at which the comparison is well posed for ANY fp32 evaluation: the oracle's own recursion run in fp32 on the CPU (the
    kernels' additions, in the kernels' order) decodes the fp64 paths and scores within the tolerance (both asserted below, without the
    GPU).  That is a property of the inputs, not of the kernels: of 25 seeds tried on the CPU, 12 had one to four decisions of the fp64
    oracle inside the rounding of a 10 000-step fp32 running sum, and at 8 of the other 13 the fp32 oracle's score missed the bound (by up
    to 2.3 x; 0.21 x and 0.38 x of the bound at this seed)."""
    B, C = 2, 4
    lengths = [L, 5000]
    g = torch.Generator().manual_seed(3004)
    feats = torch.randn(B, 10241, C, generator=g)[:, :L].contiguous()
    trans = _mask_table(torch.randn(C, C, generator=g))
    rs, rp = _oracle_viterbi(feats, lengths, trans)
    mask = R.create_mask(L, torch.as_tensor(lengths)).float()
    rs32, rp32 = R.crf_viterbi(feats, mask, torch.eye(C), torch.zeros(C), trans)
    assert rp32 == rp, 'the fp64 oracle has a decision inside fp32 rounding at this seed: the comparison would not be well posed'
    _close(rs32, rs, 5e-5, 1e-3, 'score of the oracle in fp32 on the CPU')
    score, paths = _run_viterbi(ops, feats, lengths, trans)
    _close(score, rs, 5e-5, 1e-3, 'viterbi score')
    got = _paths_list(paths, lengths)
    for b in range(B):
        wrong = [t for t in range(lengths[b]) if got[b][t] != rp[b][t]]
        assert not wrong, f'document {b}: {len(wrong)} tags differ, the first at step {wrong[0]}'


# ------------------------------------------------------------------------------------------------ 4. optional operands
@pytest.mark.parametrize('C', [4, 5])
def test_crf_optional_operands(ops, C):
    """lengths == NULL, a tag row wider than the emission row (Lt > L, what rnn_taggers passes when the batch is shorter than the padded
    targets), dfeats == NULL (BiRnnCrf.loss under no_grad) and dfeats without dtrans: each against the plain call, bit for bit."""
    B, L = 5, 19
    g = torch.Generator().manual_seed(4000 + C)
    lengths = [L, 7, 1, 0, 12]
    feats = torch.randn(B, L, C, generator=g)
    trans = _mask_table(torch.randn(C, C, generator=g))
    tags = _gold_tags(B, L, C, lengths, g)
    loss, df, dt, score, paths = _check_all(ops, feats, tags, lengths, trans)

    # lengths == NULL: every document is L long
    full = [L] * B
    tags_full = _gold_tags(B, L, C, full, g)
    loss_f, df_f, dt_f, score_f, paths_f = _check_all(ops, feats, tags_full, full, trans)
    loss_n, df_n, dt_n = _run_nll(ops, feats, tags_full, None, trans)
    score_n, paths_n = _run_viterbi(ops, feats, None, trans)
    _same_bits(loss_n, loss_f, 'loss, lengths=None')
    _same_bits(df_n, df_f, 'dfeats, lengths=None')
    _same_bits(dt_n, dt_f, 'dtrans, lengths=None')
    _same_bits(score_n, score_f, 'viterbi score, lengths=None')
    assert torch.equal(paths_n, paths_f)

    # Lt = L + 5; the extra columns and every position past a document's length hold the valid tag 1 (0 in the plain call): a wrong row
    # stride or a read past the length changes numbers instead of reading out of bounds
    wide = torch.ones(B, L + 5)
    for b, n in enumerate(lengths):
        wide[b, :n] = tags[b, :n]
    loss_w, df_w, dt_w = _run_nll(ops, feats, wide, lengths, trans)
    _same_bits(loss_w, loss, 'loss, Lt > L')
    _same_bits(df_w, df, 'dfeats, Lt > L')
    _same_bits(dt_w, dt, 'dtrans, Lt > L')

    # no gradient requested: the same loss
    loss_e, _, _ = _run_nll(ops, feats, tags, lengths, trans, want_df=False, want_dt=False)
    _same_bits(loss_e, loss, 'loss, dfeats=None')

    # dfeats without dtrans: the same dfeats (and the same loss)
    loss_d, df_d, _ = _run_nll(ops, feats, tags, lengths, trans, want_dt=False)
    _same_bits(loss_d, loss, 'loss, dtrans=None')
    _same_bits(df_d, df, 'dfeats, dtrans=None')


# ------------------------------------------------------------------------------------------------ 5. range edge of the scaled recursion
def _range_case(C):
    B, L = 8, 64
    g = torch.Generator().manual_seed(5000 + C)
    lengths = [L, L, L, L, 50, 33, 17, L]
    feats = (torch.rand(B, L, C, generator=g) * 2 - 1) * 30
    trans = _mask_table((torch.rand(C, C, generator=g) * 2 - 1) * 10)
    tags = _gold_tags(B, L, C, lengths, g)
    return feats, tags, lengths, trans


@pytest.mark.parametrize('C', [4, 5])
def test_crf_nll_at_the_edge_of_the_scaled_recursion(ops, C):
    """crf_nll4_kernel carries softmax(alpha) in fp32: it is exact to rounding while a step's worst filtered-probability ratio
    exp(-(2 Se + 2 St)) stays a normal fp32, i.e. above exp(-87.3).  Emissions uniform in +-30 and transitions uniform in +-10 put it at
    exp(-80).  C = 5 sends inputs drawn the same way through the generic log-domain kernel, which has no such limit.  Loss to 2e-6 relative
    (test_crf_long_documents).

    Gradients: C = 4 meets the tolerances of test_crf_nll_viterbi (measured on an MI355X: dfeats 8.3e-8 absolute, 0.075 of the limit).  The
    log-domain kernel does not, and no fp32 log-domain evaluation does: alpha and beta reach 1e3 here, where one fp32 ulp is 6e-5 to 1.2e-4
    and a marginal exp(alpha + beta - log Z) inherits it.  The oracle's own functions on fp32 CPU tensors are off the fp64 oracle by
    2.36e-5 absolute in dfeats on these C = 5 inputs (1.02e-5 on the C = 4 ones); the bound for C = 5 is four times that, 9.4e-5 (four: the
    summation order differs), next to the same rtol.  Measured on an MI355X: 7.6e-6."""
    feats, tags, lengths, trans = _range_case(C)
    ref_loss, ref_df, ref_dt, _ = _oracle_nll(feats, tags, lengths, trans)
    l32, df32, dt32, _ = _oracle_nll(feats, tags, lengths, trans, dtype=torch.float32)
    print(f'C = {C}: the oracle in fp32 on the CPU: loss {abs(float(l32) - float(ref_loss)) / abs(float(ref_loss)):.2e} rel, '
          f'dfeats {float((df32.double() - ref_df).abs().max()):.2e} abs, dtrans {float((dt32.double() - ref_dt).abs().max()):.2e} abs')
    loss, df, dt = _run_nll(ops, feats, tags, lengths, trans)
    print(f'loss {float(loss):.9g}, oracle {float(ref_loss):.9g}, rel {abs(float(loss) - float(ref_loss)) / abs(float(ref_loss)):.2e}')
    print(f'dfeats max err {float((df.double() - ref_df).abs().max()):.3e}, dtrans max err {float((dt.double() - ref_dt).abs().max()):.3e}')
    assert abs(float(loss) - float(ref_loss)) < 2e-6 * abs(float(ref_loss)), (float(loss), float(ref_loss))
    tol_df = TOL_DF if C == 4 else dict(rtol=1e-3, atol=4 * 2.36e-5)
    _close(df, ref_df, msg='dfeats', **tol_df)
    _close(dt, ref_dt, msg='dtrans', **TOL_DT)


# ------------------------------------------------------------------------------------------------ 6. model level, C == 3
@pytest.mark.parametrize('dtype', ['fp32', 'bf16'])
def test_crf_model_with_a_single_tag(dtype):
    """TextSegmenter(tagset_size=1, architecture='biLSTMCRF'): C = 3, the one place the head kernels see n_out = 3 together with the CRF.
    Loss and every parameter gradient against the oracle (tolerances of test_default_hidden_size_25_recurrent); Viterbi can only answer
    tag 0 at every step of every document."""
    from multimodaltopicsegmentation_amd import TextSegmenter
    B, L, NL = 4, 23, 2
    lengths = torch.tensor([23, 9, 1, 16])
    g = torch.Generator().manual_seed(6000)
    ts = TextSegmenter(1, 50, 25, num_layers=NL, architecture='biLSTMCRF', compute_dtype=dtype).to(DEV)
    m = ts.model
    assert m.num_tags == 3
    sd = m.state_dict()
    assert sd['crf.transitions'].shape == (3, 3) and sd['crf.fc.weight'].shape == (3, 50)
    p = {k: v.detach().cpu().double().requires_grad_(True) for k, v in sd.items()}
    f32 = dtype == 'fp32'
    x = torch.randn(B, L, 50, generator=g)
    y = torch.zeros(B, L)                                              # the only real tag
    h = R.rnn_forward(x.double(), lengths, p, 'model.', NL, True)
    mask = R.create_mask(h.shape[1], lengths)
    ref_loss = R.crf_nll(h, y.long()[:, :h.shape[1]], mask, p['crf.fc.weight'], p['crf.fc.bias'], p['crf.transitions'])
    loss = m.loss(x.to(DEV), lengths, y.long().to(DEV))
    ref_loss.backward()
    loss.backward()
    print(f'{dtype}: loss {loss.item():.6e}, oracle {ref_loss.item():.6e}')
    assert abs(loss.item() - ref_loss.item()) < (5e-6 if f32 else 3e-2) * max(1.0, abs(ref_loss.item()))
    grads = {n: prm.grad for n, prm in m.named_parameters()}
    worst = []
    for n in grads:
        r = p[n].grad
        if r is None:
            continue
        a = m.logical_view(grads, n).detach().cpu().double()
        assert a.shape == r.shape, n
        scale = max(float(r.abs().max()), 1e-8)
        worst.append((float((a - r).abs().max()), (3e-3 if f32 else 0.15) * scale + (2e-7 if f32 else 3e-4), n))
        full = grads[n].detach().cpu()
        assert abs(float(full.double().abs().sum()) - float(a.abs().sum())) <= 1e-6 * max(1.0, float(a.abs().sum()))   # padded units get no gradient
    for err, lim, n in worst:
        print(f'{dtype}: {n}: max err {err:.3e}, limit {lim:.3e}')
    for err, lim, n in worst:
        assert err < lim, (n, err, lim)
    # with one real tag the loss and its gradients are 0 whatever the emissions: the emissions themselves (head kernel, n_out = 3) are
    # compared too, to the logit bounds of tests/test_gpu_taggers.py (fp32 3e-5, bf16 5e-2 absolute)
    with torch.no_grad():
        feats = m.loss_and_grad(x.to(DEV), lengths, y.long().to(DEV), False)[1].float().cpu().double()
    ref_feats = (h @ p['crf.fc.weight'].t() + p['crf.fc.bias']).detach()
    for b, n in enumerate(lengths.tolist()):
        err = float((feats[b, :n] - ref_feats[b, :n]).abs().max())
        assert err < (3e-5 if f32 else 5e-2), (b, err)
    score, paths = m(x.to(DEV), lengths)
    assert paths == [[0] * n for n in lengths.tolist()]
    rs, rp = R.crf_viterbi(h.detach(), mask, p['crf.fc.weight'].detach(), p['crf.fc.bias'].detach(), p['crf.transitions'].detach())
    assert rp == paths and tuple(score.shape) == (B,)
