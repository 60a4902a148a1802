"""CPU-only: the NumPy restatement of the reference's ``mfcc`` encoder (tests/mfcc_oracle.py) against SciPy and np.pad where those define a
piece of it, the host tables of multimodaltopicsegmentation_amd/audio.py against the restatement's (each built by its own code), and the
host side of ResidentAudio, uniform_spans and load_wav."""
import cmath
import math

import numpy as np
import pytest

from tests import mfcc_oracle as O


def _ulp_close(a, b):
    """elementwise |a - b| within one fp32 ulp at their magnitude (an entry whose exact value is 0 may differ by the fp64 rounding of its
    argument: 1e-15 absolute)"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    ulp = np.spacing(np.maximum(np.abs(a), np.abs(b)).astype(np.float32)).astype(np.float64)
    return bool((np.abs(a - b) <= np.maximum(ulp, 1e-15)).all())


# ---- the restatement ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('T', [9, 10, 16, 98])
def test_delta_is_scipys_savgol_filter(T):
    signal = pytest.importorskip('scipy.signal')
    x = np.random.default_rng(T).standard_normal((T, 7)) * 30.0
    want = signal.savgol_filter(x, 9, polyorder=1, deriv=1, axis=0, mode='interp')
    assert np.abs(O.delta(x) - want).max() < 1e-12


def test_delta_is_zero_below_nine_frames():
    for T in range(1, 9):
        assert not O.delta(np.ones((T, 3)) * np.arange(T)[:, None]).any()


def test_dct_is_scipys_orthonormal_dct2():
    fft = pytest.importorskip('scipy.fft')
    x = np.random.default_rng(5).standard_normal((11, 128))
    for n_mfcc, n_mels in ((50, 128), (13, 40)):
        want = fft.dct(x[:, :n_mels], type=2, norm='ortho', axis=1)[:, :n_mfcc]
        assert np.abs(x[:, :n_mels] @ O.dct_matrix(n_mfcc, n_mels).T - want).max() < 1e-12


@pytest.mark.parametrize('n', [1, 700, 1500, 4096, 5000])
def test_framing_is_np_pad_reflect(n):
    y = np.random.default_rng(n).standard_normal(n)
    padded = np.pad(y, O.N_FFT // 2, mode='reflect')
    frames = O.frame_signal(y)
    assert frames.shape == (1 + n // O.HOP, O.N_FFT)
    for t in range(frames.shape[0]):
        assert np.array_equal(frames[t], padded[t * O.HOP:t * O.HOP + O.N_FFT])


def test_mel_table_is_slaneys():
    fb = O.mel_matrix()
    assert fb.shape == (128, 1025)
    area = fb.sum(axis=1) * (O.SR / O.N_FFT)                      # a filter of unit area in Hz, sampled every sr / n_fft
    print('filter areas', area.min(), area.max())
    assert np.abs(area - 1.0).max() < 0.011
    f = np.array(O.mel_centres())
    low, high = f[f <= 1000.0], f[f >= 1000.0]
    assert low.size > 10 and high.size > 10 and f[0] == 0.0 and abs(f[-1] - 8000.0) < 1e-9
    assert np.abs(np.diff(low) - np.diff(low)[0]).max() < 1e-9    # linear below 1 kHz
    ratio = high[1:] / high[:-1]
    assert np.abs(ratio - ratio[0]).max() < 1e-12                 # geometric above
    step_mel = O.slaney_mel(8000.0) / 129
    assert abs(np.diff(low)[0] - 200.0 / 3.0 * step_mel) < 1e-9 and abs(math.log(ratio[0]) - math.log(6.4) / 27.0 * step_mel) < 1e-12
    assert (fb.max(axis=1) > 0).all()                             # no empty filter
    assert ((fb > 0).sum(axis=0) <= 2).all()                      # every FFT bin feeds at most two filters
    assert int((fb.astype(np.float32) > 0).sum()) == 2020


def test_the_fp32_restatement_stays_in_single_precision_and_near_the_fp64_one():
    """the yardstick of the GPU tests: the figures the corpus gives on the host"""
    for (name, y), r64, r32 in zip(O.sentences(), O.reference('float64'), O.reference('float32')):
        assert all(a.dtype == np.float32 for a in r32) and all(a.dtype == np.float64 for a in r64)
        err = float(np.abs(r64[2] - r32[2]).max())
        print(f'{name}: T {r64[0].shape[0]}, host fp32 error of the statistics {err:.2e}, largest {np.abs(r64[2]).max():.1f}')
        assert err < (1e-4 if name in ('gap', 'tone', 'quiet') else 1e-5), name
    shares = {name: O.clamped_share(y) for name, y in O.sentences() if name in ('gap', 'tone')}
    print('share of dB values on the clamp', shares)
    assert 0.2 < shares['gap'] < 0.4 and shares['tone'] > 0.75


def test_corpus_holds_the_lengths_the_kernels_branch_on():
    waves, spans, names = O.corpus()
    lengths = {n: b - a for doc, nm in zip(spans, (names[:5], names[5:10], names[10:])) for (a, b), n in zip(doc, nm)}
    assert [lengths[k] for k in ('n4096', 'n4607', 'n4608', 'n8000', 'n50000', 'long300000')] == [4096, 4607, 4608, 8000, 50000, 300000]
    assert all(doc[i][1] == doc[i + 1][0] for doc in spans[:2] for i in range(3))          # touching spans
    assert any(a % 2 for doc in spans for a, _ in doc)
    assert not waves[1][78777:86777].any()


# ---- audio.py's tables against the restatement's ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n_fft,n_mels,n_mfcc', [(2048, 128, 50), (2048, 40, 13), (512, 40, 13)])
def test_host_tables_equal_the_restatements(n_fft, n_mels, n_mfcc):
    from multimodaltopicsegmentation_amd import audio
    t = audio.mfcc_tables(16000, n_fft, n_mels, n_mfcc)
    assert all(v.dtype == (np.int32 if k in ('mel_first', 'mel_ptr') else np.float32) for k, v in t.items())
    assert _ulp_close(t['window'], O.hann(n_fft))
    tw = np.array([[z.real, z.imag] for z in (cmath.exp(-2j * math.pi * m / n_fft) for m in range(n_fft))])
    assert t['twiddle'].shape == (n_fft, 2) and _ulp_close(t['twiddle'], tw)
    assert t['dct'].shape == (n_mfcc, n_mels) and _ulp_close(t['dct'], O.dct_matrix(n_mfcc, n_mels))
    want = O.mel_matrix(16000, n_fft, n_mels)
    dense = np.zeros(want.shape, dtype=np.float32)
    first, ptr, w = t['mel_first'], t['mel_ptr'], t['mel_w']
    assert first.shape == (n_mels,) and ptr.shape == (n_mels + 1,) and ptr[0] == 0 and ptr[-1] == w.size and (np.diff(ptr) >= 1).all()
    for m in range(n_mels):
        dense[m, first[m]:first[m] + ptr[m + 1] - ptr[m]] = w[ptr[m]:ptr[m + 1]]
    assert _ulp_close(dense, want) and np.array_equal(dense > 0, want.astype(np.float32) > 0)
    if (n_fft, n_mels) == (2048, 128):
        assert w.size == 2020 and (w > 0).all()
    assert audio.mfcc_tables(16000, n_fft, n_mels, n_mfcc) is t                      # cached per parameter set


def test_tables_refuse_what_the_kernels_refuse():
    from multimodaltopicsegmentation_amd import audio
    for bad in (1000, 32, 8192):
        with pytest.raises(ValueError):
            audio.mfcc_tables(16000, bad, 40, 13)
    with pytest.raises(ValueError):
        audio.mfcc_tables(16000, 2048, 40, 41)
    with pytest.raises(ValueError, match='empty'):
        audio.mfcc_tables(16000, 64, 128, 13)


# ---- ResidentAudio on the host ---------------------------------------------------------------------------------------------------------------
def _waves():
    rng = np.random.default_rng(3)
    return [rng.standard_normal(40000).astype(np.float32), rng.standard_normal(20000).astype(np.float64)]


def test_resident_audio_host_tables():
    from multimodaltopicsegmentation_amd import ResidentAudio
    spans = [[(0.0, 0.5), (0.50001, 1.3), (1.3, 9.0)], [(0.1, 0.9)]]
    a = ResidentAudio(_waves(), spans, 'cpu')
    assert len(a) == a.n_docs == 2 and a.total_sentences == 4 and a.total_samples == 60000
    assert a.sentences.tolist() == [3, 1]
    # int(sr * t) truncates: 0.50001 s is sample 8000, not 8001; 9.0 s is clipped to the document's 40 000 samples
    assert a.sample_counts.tolist() == [8000, int(16000 * 1.3) - 8000, 40000 - int(16000 * 1.3), 12800]
    assert a._start_host.tolist() == [0, 8000, int(16000 * 1.3), 40000 + 1600]
    assert a.frame_counts.tolist() == [1 + n // 512 for n in a.sample_counts.tolist()] and a.total_frames == int(a.frame_counts.sum())
    assert a.wave is None and a.nbytes == 0
    with pytest.raises(RuntimeError):
        a.mfcc()
    b = ResidentAudio(_waves(), [[(0, 8000), (8000, 20800), (20800, 144000)], [(1600, 14400)]], 'cpu', unit='samples')
    assert b.sample_counts.tolist() == a.sample_counts.tolist() and b._start_host.tolist() == a._start_host.tolist()


def test_resident_audio_names_the_document_and_the_sentence():
    from multimodaltopicsegmentation_amd import ResidentAudio
    w = _waves()
    ok = [[(0.0, 1.0)], [(0.0, 1.0)]]
    with pytest.raises(ValueError, match='document 1 has no samples'):
        ResidentAudio([w[0], np.zeros(0, dtype=np.float32)], ok, 'cpu')
    with pytest.raises(ValueError, match='wave of document 1 is 2-d'):
        ResidentAudio([w[0], np.zeros((2, 20000), dtype=np.float32)], ok, 'cpu')
    with pytest.raises(ValueError, match='sentence 1 of document 1 is empty'):
        ResidentAudio(w, [[(0.0, 1.0)], [(0.0, 1.0), (1.25, 1.5)]], 'cpu')                # starts at the document's end after clipping
    with pytest.raises(ValueError, match='sentence 0 of document 0 is empty'):
        ResidentAudio(w, [[(1.0, 1.0)], [(0.0, 1.0)]], 'cpu')
    with pytest.raises(ValueError, match='sentence 2 of document 0 has 4095 samples.*librosa.*9 frames.*reference raises'):
        ResidentAudio(w, [[(0, 5000), (5000, 9096), (9096, 13191)], [(0, 5000)]], 'cpu', unit='samples')
    ResidentAudio(w, [[(0, 5000), (5000, 9096), (9096, 13192)], [(0, 5000)]], 'cpu', unit='samples')   # 4096 samples are 9 frames
    with pytest.raises(ValueError, match='sentence 0 of document 1 has 19000 samples'):   # clipped from 30 000 to the document's 20 000
        ResidentAudio(w, [[(0, 40000)], [(1000, 30000)]], 'cpu', unit='samples').mfcc(hop=4096)
    with pytest.raises(ValueError, match='sentence 0 of document 1 starts at sample -1'):
        ResidentAudio(w, [[(0, 5000)], [(-1, 5000)]], 'cpu', unit='samples')
    with pytest.raises(ValueError):
        ResidentAudio(w, ok[:1], 'cpu')
    with pytest.raises(ValueError):
        ResidentAudio(w, ok, 'cpu', unit='frames')


def test_uniform_spans_are_upstreams_units():
    from multimodaltopicsegmentation_amd import uniform_spans

    def to_sample(sr, t):                       # extract_embeddings_inference.py's conversion
        return int(sr * t)
    for n, interval in ((16000 * 7 + 123, 1.0), (100000, 0.5), (50000, 2.0), (15999, 1.0)):
        audio_length = n / 16000
        want = [(to_sample(16000, interval * i), to_sample(16000, interval * i + 1)) for i in range(int(audio_length // interval))]
        assert uniform_spans(n, interval) == want
    assert uniform_spans(100000, 0.5)[3] == (24000, 40000)          # the window is one second whatever the interval
    assert uniform_spans(15999) == []


def test_load_wav_round_trip(tmp_path):
    wavfile = pytest.importorskip('scipy.io.wavfile')
    from multimodaltopicsegmentation_amd import load_wav
    rng = np.random.default_rng(9)
    pcm = rng.integers(-32768, 32768, size=5000).astype(np.int16)
    flt = rng.standard_normal(3000).astype(np.float32) * 0.1
    wavfile.write(tmp_path / 'a.wav', 16000, pcm)
    wavfile.write(tmp_path / 'b.wav', 16000, flt)
    wavfile.write(tmp_path / 'rate.wav', 8000, pcm)
    wavfile.write(tmp_path / 'stereo.wav', 16000, np.stack([pcm, pcm], axis=1))
    a, b = load_wav(str(tmp_path), ['a', 'b.wav'])
    assert a.dtype == b.dtype == np.float32 and np.array_equal(a, pcm.astype(np.float32) / 32768.0) and np.array_equal(b, flt)
    with pytest.raises(ValueError, match='8000 Hz'):
        load_wav(str(tmp_path), ['rate'])
    with pytest.raises(ValueError, match='2 channels'):
        load_wav(str(tmp_path), ['stereo'])
