"""Prosodic sentence features on the GPU (csrc/prosody.hip, audio.ResidentAudio.pitch / yin / prosodic, ResidentCorpus.with_prosodic).

The checker is the NumPy restatement of tests/prosody_oracle.py.  The tests are STAGED: every stage is checked given the DEVICE's output of
the stage before it, so a threshold crossed upstream can neither hide nor fake an error downstream.
  cmnd / shift   against the fp64 restatement: per sentence, the device's error must stay within K times the error of the SAME restatement
                 run in fp32 plus 2 ulp of the sentence's largest value (the MFCC suite's rule).  K is twice the largest ratio measured
                 on an MI355X, capped at 8.
  observe        from the device's cmnd / shift: voiced_prob within 4 ulp (fp32), the same set of non-floor bins per frame.
  Viterbi        from the device's log-observations: the state path EXACTLY the dense NumPy fp64 path over the package's tables, f0 and
                 flags with it; constructed log-observations pin the tie rule (the first of equals) and the jump out of the band.
  pick, stats    from the device's tracks: the plain-YIN f0 bit for bit (one fp32 add, one correctly rounded division); the scalar
                 columns within 2 ulp (fp32) of the fp64 statistics -- the kernel accumulates in fp64 in another order (relative 2^-53 T)
                 and rounds once, which is half an ulp; pitch_jump the same plus 1e-13 for the difference of two ratios near 1.
  delta          the bits of mts_mfcc_frames' delta on the same fp32 input, and within 2 ulp of the largest input of the fp64 slope.
  end to end     audio.prosodic() equals the staged composition bit for bit, whatever the chunking; bf16 is one rounding of the fp32 row;
                 nothing outside the 167 columns is written.

Largest ratios of device error to host-fp32 error measured on an MI355X (13 sentences, 199 frames):
  cmnd    0.96 at fmin 70, fmax 500 (v4096); 1.23 at 200 - 400 (d1first)                                              -> K = 2.5
  shift   2.28 at 70 - 500; 2.74 at 200 - 400 (d1first: host 1.0e-7, device 2.8e-7 on shifts up to 0.99; 2.62 on noise) -> K = 5.5
The shift is a quotient of two second differences of cmnd: where the curvature is small it amplifies the last bits of cmnd on the host
and on the device alike, which is why its errors are 1e-7 .. 1e-4 on both sides and its ratio the larger one."""
import numpy as np
import pytest
import torch

from tests import mfcc_oracle as MO
from tests import prosody_oracle as PO
from tests.test_pca_cpu import corpus_of

pytestmark = pytest.mark.gpu
DEV = 'cuda'
F32, BF16 = torch.float32, torch.bfloat16
K = {'cmnd': 2.5, 'shift': 5.5}                  # twice the largest measured ratio of the stage (the cap is 8)
SENTINEL = -12288.0
SETS = [(70.0, 500.0), (200.0, 400.0)]
_cache = {}


def _ulp(v):
    return float(np.spacing(np.float32(abs(float(v)))))


def _audio():
    if 'audio' not in _cache:
        from multimodaltopicsegmentation_amd import ResidentAudio
        waves, spans, _ = PO.corpus()
        _cache['audio'] = ResidentAudio(list(waves), [list(s) for s in spans], DEV, unit='samples')
    return _cache['audio']


def _tabs(fmin, fmax):
    """-> (the package's host tables, the same with the arrays on the device)"""
    from multimodaltopicsegmentation_amd import pyin_tables
    host = pyin_tables(PO.SR, fmin, fmax)
    return host, {k: torch.from_numpy(v).to(DEV) if isinstance(v, np.ndarray) else v for k, v in host.items()}


def _frame_start(a):
    start = np.concatenate([[0], np.cumsum(a.frame_counts)]).astype(np.int64)
    return start, torch.from_numpy(start).to(DEV)


def _staged(fmin, fmax):
    """every stage of the whole test corpus through the C ABI, once per parameter set"""
    key = ('staged', fmin, fmax)
    if key not in _cache:
        from multimodaltopicsegmentation_amd import ops
        a = _audio()
        host, tabs = _tabs(fmin, fmax)
        start, fs = _frame_start(a)
        cmnd, shift = ops.yin_frames(a.wave, a.sent_start, a.sent_len, fs, a.total_frames, host['min_period'], host['max_period'])
        vp, logobs = ops.pyin_observe(cmnd, shift, tabs)
        state, f0, voiced = ops.pyin_viterbi(logobs, fs, tabs)
        yin_f0 = ops.yin_pick(cmnd, shift, host['min_period'], PO.SR)
        _cache[key] = dict(host=host, tabs=tabs, start=start, fs=fs, cmnd=cmnd, shift=shift, vp=vp, logobs=logobs, state=state, f0=f0,
                           voiced=voiced, yin_f0=yin_f0)
    return _cache[key]


def _doc_first(a):
    first = np.zeros(a.total_sentences, dtype=np.uint8)
    first[np.concatenate([[0], np.cumsum(a.sentences)[:-1]])] = 1
    return first


# ---- stage 1 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('fmin,fmax', SETS, ids=['70-500', '200-400'])
def test_cmnd_and_shift_match_the_fp64_restatement(fmin, fmax):
    st = _staged(fmin, fmax)
    a = _audio()
    assert a.total_sentences == 13 and a.frame_counts.min() == 9 and a.frame_counts.max() == 24
    got_c, got_s = st['cmnd'].cpu().numpy().astype(np.float64), st['shift'].cpu().numpy().astype(np.float64)
    assert got_c.shape == (a.total_frames, st['host']['n_lags']) == got_s.shape
    ratios, ok = {'cmnd': {}, 'shift': {}}, True
    for s, ((name, _, _, _), r64, r32) in enumerate(zip(PO.sentences(), PO.reference_cmnd('float64', fmin, fmax),
                                                        PO.reference_cmnd('float32', fmin, fmax))):
        rows = slice(st['start'][s], st['start'][s + 1])
        for what, got, k in (('cmnd', got_c, 0), ('shift', got_s, 1)):
            host, err = float(np.abs(r32[k] - r64[k]).max()), float(np.abs(got[rows] - r64[k]).max())
            ratios[what][name] = err / max(host, 1e-300)
            print(f'{what} {name}: device {err:.3e}, host fp32 {host:.3e}, ratio {ratios[what][name]:.2f}, largest {np.abs(r64[k]).max():.3f}')
            ok &= err <= K[what] * host + 2 * _ulp(np.abs(r64[k]).max())
    for what in ratios:
        print(f'{what} {fmin:g}-{fmax:g}: largest ratio', max(ratios[what].values()))
    assert ok, ratios
    silent = [n for n, *_ in PO.sentences()].index('silent')
    rows = slice(st['start'][silent], st['start'][silent + 1])
    assert not got_c[rows].any() and not got_s[rows].any()                       # 0 / (0 + tiny) is 0, and so are the shifts


# ---- stage 2 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('fmin,fmax', SETS, ids=['70-500', '200-400'])
def test_observations_follow_from_the_devices_cmnd(fmin, fmax):
    st = _staged(fmin, fmax)
    nb, floor = st['host']['n_bins'], st['host']['log_floor']
    c, sh = st['cmnd'].cpu().numpy(), st['shift'].cpu().numpy()
    vp, lo = st['vp'].cpu().numpy(), st['logobs'].cpu().numpy()
    assert vp.dtype == np.float32 and lo.dtype == np.float64 and lo.shape == (c.shape[0], 2 * nb)
    worst, voiced_frames = 0.0, 0
    for f in range(c.shape[0]):
        want_vp, obs = PO.observe(c[f], sh[f], fmin, fmax)
        worst = max(worst, abs(float(vp[f]) - float(np.float32(want_vp))) / _ulp(max(want_vp, 2.0 ** -126)))
        assert np.array_equal(lo[f, :nb] != floor, obs > 0.0), f
        hit = obs > 0.0
        assert np.allclose(np.exp(lo[f, :nb][hit]), obs[hit], rtol=1e-10, atol=0.0), f
        assert np.all(lo[f, nb:] == lo[f, nb]) and lo[f, nb] <= 0.0 and np.isfinite(lo[f, nb]), f
        if want_vp < 1.0 - 1e-6:      # where 1 - voiced_prob keeps its digits
            assert abs(lo[f, nb] - np.log((1.0 - want_vp) / nb)) <= 1e-9, f
        voiced_frames += want_vp >= 0.5
    print(f'voiced_prob {fmin:g}-{fmax:g}: largest difference {worst:.2f} ulp; {voiced_frames} of {c.shape[0]} frames at or above 0.5')
    assert worst <= 4.0
    assert 0 < voiced_frames < c.shape[0]


# ---- stage 3 ---------------------------------------------------------------------------------------------------------------------------
def _check_paths(host, logobs, start, state, f0, voiced):
    nb = host['n_bins']
    for s in range(len(start) - 1):
        rows = slice(start[s], start[s + 1])
        want = PO.viterbi(logobs[rows], host['ltri'], host['lsrc'], host['linit'], host['log_floor'])
        assert np.array_equal(state[rows], want), (s, state[rows].tolist(), want.tolist())
        want_f0 = np.where(want < nb, host['freqs'][want % nb], np.float32(np.nan)).astype(np.float32)
        assert np.array_equal(f0[rows], want_f0, equal_nan=True) and np.array_equal(voiced[rows] != 0, want < nb)


@pytest.mark.parametrize('fmin,fmax', SETS, ids=['70-500', '200-400'])
def test_viterbi_path_is_the_numpy_fp64_path(fmin, fmax):
    st = _staged(fmin, fmax)
    state, f0, voiced = (st[k].cpu().numpy() for k in ('state', 'f0', 'voiced'))
    assert state.dtype == np.int32 and f0.dtype == np.float32 and voiced.dtype == np.uint8
    _check_paths(st['host'], st['logobs'].cpu().numpy(), st['start'], state, f0, voiced)
    assert 0 < int(voiced.sum()) < voiced.shape[0]


@pytest.mark.parametrize('fmin,fmax', SETS, ids=['70-500', '200-400'])
def test_viterbi_ties_and_jumps_out_of_the_band(fmin, fmax):
    """constructed log-observations: all equal (every step is a tie between the sources the symmetric triangle treats alike), small
    integers (exact ties between different routes), and one voiced bin per frame that leaps across the band while every other state sits
    on the floor (the dense walk)"""
    from multimodaltopicsegmentation_amd import ops
    host, tabs = _tabs(fmin, fmax)
    nb, floor = host['n_bins'], host['log_floor']
    rng = np.random.default_rng(3)
    flat = np.zeros((5, 2 * nb))
    ints = -rng.integers(0, 3, size=(9, 2 * nb)).astype(np.float64)
    leap = np.full((7, 2 * nb), floor)
    for t, b in enumerate((10, 12, nb - 3, nb - 8, nb // 3, nb // 3, 0)):
        leap[t, b] = 0.0
    both = np.full((6, 2 * nb), floor)                                    # two equal tracks: the lower index must win
    both[:, 7] = both[:, nb - 9] = -1.0
    logobs = np.concatenate([flat, ints, leap, both])
    start = np.array([0, 5, 14, 21, 27], dtype=np.int64)
    state, f0, voiced = ops.pyin_viterbi(torch.from_numpy(logobs).to(DEV), torch.from_numpy(start).to(DEV), tabs)
    _check_paths(host, logobs, start, state.cpu().numpy(), f0.cpu().numpy(), voiced.cpu().numpy())
    assert state.cpu().numpy()[21:27].tolist() == [7] * 6
    assert state.cpu().numpy()[14:21].tolist()[:2] == [10, 12]


# ---- stage 4 ---------------------------------------------------------------------------------------------------------------------------
def test_plain_yin_pick_is_bitwise():
    for fmin, fmax in SETS:
        st = _staged(fmin, fmax)
        want = PO.yin_pick(st['cmnd'].cpu().numpy(), st['shift'].cpu().numpy(), st['host']['min_period'])
        assert want.dtype == np.float32 and np.array_equal(st['yin_f0'].cpu().numpy(), want, equal_nan=True)
    # constructed rows: the threshold decides between two troughs; equal minima (the first wins); a trough on the last lag and on lag 0;
    # a flat row (no trough: lag 0)
    from multimodaltopicsegmentation_amd import ops
    c = np.ones((5, 198), dtype=np.float32)
    c[0, 5], c[0, 20] = 0.3, 0.05
    c[1, 7] = c[1, 30] = 0.2
    c[2, 197] = 0.05
    c[3, 0] = 0.05
    sh = np.random.default_rng(8).uniform(-0.5, 0.5, c.shape).astype(np.float32)
    picks = {}
    for th in (0.1, 0.5):
        picks[th] = ops.yin_pick(torch.from_numpy(c).to(DEV), torch.from_numpy(sh).to(DEV), 32, PO.SR, th).cpu().numpy()
        assert np.array_equal(picks[th], PO.yin_pick(c, sh, 32, threshold=th))
    lag = lambda th, r: np.float32(PO.SR) / picks[th][r] - sh[r, [20, 7, 197, 0, 0][r] if th == 0.1 else [5, 7, 197, 0, 0][r]]
    assert [round(float(lag(0.1, r))) for r in range(5)] == [52, 39, 229, 32, 32]
    assert [round(float(lag(0.5, r))) for r in range(5)] == [37, 39, 229, 32, 32]


def _check_scalars(got, f0, vp, prev, start, first, names):
    worst = 0.0
    for s in range(len(start) - 1):
        rows = slice(start[s], start[s + 1])
        before = None if s == 0 else prev[start[s - 1]:start[s]]
        want = PO.scalar_stats(f0[rows], vp[rows], before, bool(first[s]))
        for k in range(7):
            slack = 2 * _ulp(max(abs(want[k]), 2.0 ** -126)) + (1e-13 if k == 6 else 0.0)
            worst = max(worst, abs(float(got[s, k]) - want[k]) / slack)
            assert abs(float(got[s, k]) - want[k]) <= slack, (names[s], k, float(got[s, k]), want[k])
    return worst


def test_scalar_statistics_follow_from_the_devices_tracks():
    from multimodaltopicsegmentation_amd import ops
    a, st = _audio(), _staged(*SETS[0])
    names = [n for n, *_ in PO.sentences()]
    first = _doc_first(a)
    out = torch.full((a.total_sentences, 9), SENTINEL, device=DEV)
    ops.prosodic_stats(st['f0'], st['vp'], st['yin_f0'], st['fs'], torch.from_numpy(first).to(DEV), out, 7)
    got = out.cpu().numpy()
    assert np.all(got[:, 6] == SENTINEL) and np.all(got[:, 8] == SENTINEL)
    cols = got[:, [0, 1, 2, 3, 4, 5, 7]]
    f0, vp, prev = (st[k].cpu().numpy() for k in ('f0', 'vp', 'yin_f0'))
    print('scalars: largest error over its bound', _check_scalars(cols, f0, vp, prev, st['start'], first, names))
    silent, d1 = names.index('silent'), names.index('d1first')
    assert np.all(cols[silent] == [0.0, 0.0, a.frame_counts[silent], 0.0, 0.0, 0.0, 0.0])       # no voiced frame: NaN -> 0, one open run
    assert cols[d1, 6] == 0.0 and cols[0, 6] == 0.0 and first.sum() == 2                        # the track resets per document
    assert np.count_nonzero(cols[:, 6]) >= 8 and np.count_nonzero(cols[:, 3]) >= 1              # jumps elsewhere; a sentence with two pauses
    # constructed tracks: every branch of the pause rule, a NaN-only neighbour, and runs that cross the 64-frame chunks of the kernel
    rng = np.random.default_rng(9)
    T = [9, 70, 130, 64, 65, 12, 200, 10]
    start = np.concatenate([[0], np.cumsum(T)]).astype(np.int64)
    vp2 = rng.random(int(start[-1])).astype(np.float32)
    vp2[start[1]:start[2]] = np.repeat(rng.random(18), 4)[:70].astype(np.float32)
    vp2[start[2]:start[2] + 100], vp2[start[2] + 100:start[3]] = 0.25, 0.9                       # one pause of 100 frames, closed
    vp2[start[3]:start[4]] = 0.9                                                                 # no pause frame
    vp2[start[4]:start[5]] = 0.1                                                                 # all pause
    vp2[start[5]:start[5] + 6], vp2[start[5] + 6:start[6]] = 0.8, 0.2                            # a trailing pause only
    vp2[start[7]:start[8]] = 0.5                                                                 # exactly 0.5 is voiced
    f2 = np.where(vp2 >= 0.5, rng.uniform(80, 400, vp2.shape[0]), np.nan).astype(np.float32)
    prev2 = rng.uniform(80, 400, vp2.shape[0]).astype(np.float32)
    prev2[start[5]:start[6]] = np.nan                                                            # the jump after it is NaN -> 0
    first2 = np.array([1, 0, 0, 0, 0, 0, 0, 1], dtype=np.uint8)
    out2 = torch.zeros((8, 7), device=DEV)
    ops.prosodic_stats(*(torch.from_numpy(x).to(DEV) for x in (f2, vp2, prev2, start, first2)), out2, 6)
    got2 = out2.cpu().numpy()
    print('constructed: largest error over its bound', _check_scalars(got2, f2, vp2, prev2, start, first2, [f'c{i}' for i in range(8)]))
    assert got2[6, 6] == 0.0 and got2[4, 6] == 0.0 and got2[7, 6] == 0.0 and got2[5, 6] != 0.0 and got2[1, 6] != 0.0
    assert got2[4].tolist() == [0.0, 0.0, 65.0, 0.0, 0.0, 0.0, 0.0] and got2[3, 2:4].tolist() == [0.0, 0.0] and got2[2, 2] == 100.0
    half = torch.zeros((8, 7), dtype=BF16, device=DEV)
    ops.prosodic_stats(*(torch.from_numpy(x).to(DEV) for x in (f2, vp2, prev2, start, first2)), half, 6)
    assert torch.equal(half, out2.to(BF16))


# ---- stage 5 ---------------------------------------------------------------------------------------------------------------------------
def test_frame_delta_has_the_bits_of_the_mfcc_delta():
    from multimodaltopicsegmentation_amd import audio, ops
    a = _audio()
    start, fs = _frame_start(a)
    t = {k: torch.from_numpy(v).to(DEV) for k, v in audio.mfcc_tables(PO.SR, 2048, 40, 13).items()}
    mel = ops.mel_frames(a.wave, a.sent_start, a.sent_len, fs, a.total_frames, t['window'], t['twiddle'], t['mel_first'], t['mel_ptr'], t['mel_w'], 512)
    both = ops.mfcc_frames(mel, fs, t['dct'], torch.empty((a.total_frames, 26), device=DEV))
    assert torch.equal(ops.frame_delta(both[:, :13].contiguous(), fs), both[:, 13:])
    got = ops.frame_delta(mel, fs).cpu().numpy()
    x = mel.cpu().numpy()
    for s in range(a.total_sentences):
        rows = slice(start[s], start[s + 1])
        want = MO.delta(x[rows].astype(np.float64))
        assert np.abs(got[rows] - want).max() <= 2 * _ulp(np.abs(x[rows]).max())
        assert np.abs(want).max() > 0.0 or not x[rows].any()
    # fewer than nine frames: 0; an odd width; several sentences inside one workgroup's 16 frames
    T = [5, 9, 8, 3, 11]
    start2 = np.concatenate([[0], np.cumsum(T)]).astype(np.int64)
    x2 = np.random.default_rng(4).standard_normal((int(start2[-1]), 7)).astype(np.float32)
    got2 = ops.frame_delta(torch.from_numpy(x2).to(DEV), torch.from_numpy(start2).to(DEV)).cpu().numpy()
    for s, n in enumerate(T):
        rows = slice(start2[s], start2[s + 1])
        assert np.abs(got2[rows] - MO.delta(x2[rows].astype(np.float64))).max() <= 2 * _ulp(np.abs(x2[rows]).max())
        assert (n >= 9) == bool(got2[rows].any())


# ---- end to end ------------------------------------------------------------------------------------------------------------------------
def _composition():
    """the 167-wide matrix put together from the stages through the C ABI"""
    if 'rows' not in _cache:
        from multimodaltopicsegmentation_amd import audio, ops
        a, st = _audio(), _staged(*SETS[0])
        t = {k: torch.from_numpy(v).to(DEV) for k, v in audio.mfcc_tables(PO.SR, 2048, 40, 1).items()}
        fs = st['fs']
        mel = ops.mel_frames(a.wave, a.sent_start, a.sent_len, fs, a.total_frames, t['window'], t['twiddle'], t['mel_first'], t['mel_ptr'], t['mel_w'], 512)
        out = torch.empty((a.total_sentences, 167), device=DEV)
        ops.frame_pool(mel, fs, out[:, 6:86], first='mean', with_std=True)
        ops.frame_pool(ops.frame_delta(mel, fs), fs, out[:, 86:166], first='mean', with_std=True)
        ops.prosodic_stats(st['f0'], st['vp'], st['yin_f0'], fs, torch.from_numpy(_doc_first(a)).to(DEV), out, 166)
        _cache['rows'] = out
    return _cache['rows']


def test_prosodic_equals_the_staged_composition():
    a, want = _audio(), _composition()
    got = a.prosodic()
    assert got.dtype == F32 and tuple(got.shape) == (a.total_sentences, 167) and torch.equal(got, want)
    assert bool(torch.isfinite(got).all())
    assert torch.equal(a.prosodic(workspace_bytes=1), want)                       # a chunk per sentence
    assert torch.equal(a.prosodic(workspace_bytes=60 * 8400), want)               # chunks of a few sentences, cut where the budget says
    assert torch.equal(a.prosodic(out_dtype=BF16), want.to(BF16))                 # one rounding of the fp32 row
    wide = torch.full((a.total_sentences, 200), SENTINEL, device=DEV)
    assert a.prosodic(out=wide[:, 20:187]).data_ptr() == wide[:, 20:].data_ptr()
    assert torch.equal(wide[:, 20:187], want) and bool((wide[:, :20] == SENTINEL).all()) and bool((wide[:, 187:] == SENTINEL).all())
    # the mel block is the reference's: mean and std of the 40-band POWER and of its delta
    rows = want.cpu().numpy().astype(np.float64)
    for s, (name, y, _, _) in enumerate(PO.sentences()):
        mel = PO.mel40(y)
        d = MO.delta(mel)
        ref = np.concatenate([mel.mean(axis=0), mel.std(axis=0), d.mean(axis=0), d.std(axis=0)])
        assert np.abs(rows[s, 6:166] - ref).max() <= 1e-4 * max(np.abs(ref).max(), 1e-30), name


def test_pitch_and_yin_are_the_staged_tracks_and_repeat_their_bits():
    a, st = _audio(), _staged(*SETS[0])
    f0, vp, voiced = a.pitch()
    assert f0.dtype == F32 and vp.dtype == F32 and voiced.dtype == torch.bool and f0.numel() == a.total_frames
    assert torch.equal(vp, st['vp']) and torch.equal(voiced, st['voiced'] != 0)
    assert np.array_equal(f0.cpu().numpy(), st['f0'].cpu().numpy(), equal_nan=True)
    assert torch.equal(torch.isnan(f0), ~voiced)
    assert torch.equal(a.yin(), st['yin_f0'])
    again = a.pitch(workspace_bytes=1)
    assert np.array_equal(again[0].cpu().numpy(), f0.cpu().numpy(), equal_nan=True) and torch.equal(again[1], vp)
    narrow = a.pitch(fmin=200.0, fmax=400.0)
    st2 = _staged(*SETS[1])
    assert torch.equal(narrow[1], st2['vp']) and torch.equal(narrow[2], st2['voiced'] != 0)
    assert torch.equal(a.prosodic(), a.prosodic())


# ---- the corpus ------------------------------------------------------------------------------------------------------------------------
def _text_corpus(wire='fp32'):
    a = _audio()
    rows = a.sentences.tolist()
    text = np.ascontiguousarray(np.random.default_rng(5).integers(-8, 9, size=(sum(rows), 6)).astype(np.float32))
    return corpus_of(text, rows, DEV, wire=wire), a, text


def test_with_prosodic_lands_in_the_right_columns():
    corpus, a, text = _text_corpus()
    want = _composition()
    second = corpus.with_prosodic(a, field='embeddings2')
    assert corpus.corpus2 is None and torch.equal(second.corpus2, want) and torch.equal(second.corpus, corpus.corpus)
    assert torch.equal(corpus.with_prosodic(a).corpus, want)
    fused = corpus.with_prosodic(a, field='append')
    assert tuple(fused.corpus.shape) == (a.total_sentences, 6 + 167)
    assert torch.equal(fused.corpus[:, :6], corpus.corpus) and torch.equal(fused.corpus[:, 6:], want)
    b = second.batch([1, 0])
    cut = np.concatenate([[0], np.cumsum(a.sentences)])
    assert b['src_tokens2'].shape[2] == 167
    for i, d in enumerate((1, 0)):
        assert torch.equal(b['src_tokens2'][i, :int(a.sentences[d])], want[cut[d]:cut[d + 1]])
    half, _, _ = _text_corpus('bf16')
    assert torch.equal(half.with_prosodic(a, field='append').corpus[:, 6:], want.to(BF16))
    with pytest.raises(ValueError):
        corpus.with_prosodic(a, field='embeddings3')


def test_one_fit_epoch_and_evaluate_on_the_fused_corpus():
    from multimodaltopicsegmentation_amd import BiLSTMLateFusion, evaluate
    from multimodaltopicsegmentation_amd.trainer import NativeTrainer
    corpus, a, _ = _text_corpus()
    fused = corpus.with_prosodic(a, field='embeddings2')
    model = BiLSTMLateFusion(2, [6, 167], 8, num_layers=1, loss_fn='FocalLoss', compute_dtype='fp32', seed=11).to(DEV)
    record = NativeTrainer(model, lr=1e-3).fit(fused, fused, batch_size=2, max_epochs=1)
    assert len(record['epochs']) == 1 and np.isfinite(record['epochs'][0]['train_loss'])
    ev = evaluate(model, fused, batch_size=2, threshold=0.5)
    assert len(ev['per_document']['Pk']) == 2 and np.isfinite(ev['mean']['Pk'])
