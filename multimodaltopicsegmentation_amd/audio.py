"""MFCC sentence features from resident waveforms.

Every audio encoder the reference trains on is a pretrained network (x-vectors, openl3, CREPE, wav2vec, ECAPA) -- but one: ``mfcc``
(train_fit.py:245-248, ``'mfcc': 200``).  extract_acoustic_features.py:58-72 defines it: per sentence ``librosa.feature.mfcc(y, sr,
n_mfcc=50)``, its ``librosa.feature.delta``, then ``np.nanmean`` and ``np.nanstd`` over the frames of both: a 200-wide sentence vector from
nothing but the waveform and the sentence times.  Here the waveforms are uploaded ONCE and the frames are made in HBM by csrc/mfcc.hip:

  * ``ResidentAudio(waves, spans, device)`` holds the concatenated fp32 waveform and the sentence table on the device;
  * ``audio.mfcc()`` is a ``frames.ResidentFrames`` of [mfcc(50) | delta(50)] frames (``ops.mel_frames``: framing, window, FFT, mel;
    ``ops.mfcc_frames``: dB, DCT, delta);
  * ``audio.mfcc().pool('mean_std')`` -- ``audio.mfcc_stats()`` -- is, column for column, the reference's [mean x, mean dx, std x, std dx],
    and ``ResidentCorpus.with_frames(audio.mfcc(), 'mean_std', field=...)`` carries it into a corpus.

The definition is librosa 0.8.1's (the reference's requirements.txt) at the arguments the reference passes, restated: sr = 16000; frames of
n_fft = 2048 every hop = 512 samples, centred, the sentence reflect-padded about its OWN ends (T = 1 + n // hop frames); periodic Hann
window; power spectrum; 128 Slaney mel filters from 0 to sr / 2 with area normalisation; 10 log10(max(1e-10, .)) clamped 80 dB below the
sentence's largest value; orthonormal DCT-II, coefficients 0 .. 49; delta = scipy.signal.savgol_filter(x, 9, polyorder=1, deriv=1,
mode='interp') along the frames.  The arithmetic is stated in include/mts.h.

Deviations, on purpose.  Parity with librosa itself is UNPINNED: librosa cannot run where this was built, so the tests check against a NumPy
restatement of the lines above.  A non-finite sample is refused at upload (np.nanmean would skip what it made of it).  The sums run in the
kernels' fixed order.  A sentence shorter than 8 * hop = 4096 samples (0.256 s) is refused here where upstream raises (librosa's delta
needs 9 frames).

The reference's other model-free audio encoder, ``prosodic`` (train_fit.py:245, 167 wide; extract_acoustic_features.py:74-108), is built on
the same resident waveforms by csrc/prosody.hip: ``audio.pitch()`` (pYIN: f0, voicing probability, voiced flag per frame), ``audio.yin()``
(the plain-YIN track the reference keeps of the previous sentence) and ``audio.prosodic()``: [f0 mean, f0 std, pause mean, pause std,
voiced-intensity mean, voiced-intensity std | mel mean (40), mel std (40) | delta-mel mean (40), delta-mel std (40) | pitch_jump];
``ResidentCorpus.with_prosodic(audio, field=...)`` carries it into a corpus.  Its definition (librosa 0.8.1's ``pyin`` / ``yin``, restated
in include/mts.h) is UNPINNED against librosa as well, and two parts of it are RECALLED rather than read: the window-edge indexing of the
difference function and the transition width of 141 bins.  Deviations, on purpose: the difference function is the direct sum, not librosa's
FFT autocorrelation with its ``< 1e-6`` zeroing; a parabolic shift that is not finite is 0; the previous-sentence track resets at every
document, as the extractor's loop does (extract_embeddings.py:502).

The reference's learned audio encoder, wav2vec 2.0 (extract_embeddings.py:173-183), runs on the same resident waveforms from a
``Wav2Vec2Weights``: ``audio.wav2vec2(weights)`` is a ``ResidentFrames`` of ``last_hidden_state`` frames, ``audio.wav2vec2_stats(weights,
mode)`` their pooled matrix without keeping the frames (wav2vec2.py, csrc/wav2vec2.hip).  Its shortest sentence is 400 samples:
``ResidentAudio(..., min_samples=400)`` lowers the constructor's bound, which the framed features above then apply when they are called.
"""
import os

import numpy as np
import torch

from .frames import ResidentFrames

_CHECK_SAMPLES = 1 << 22                   # samples per slice of the upload's finiteness check
_DELTA_FRAMES = 9                          # librosa.feature.delta's default width: it raises for fewer frames
_TABLES = {}                               # (sr, n_fft, n_mels, n_mfcc) -> the host tables


def _hz_to_mel(f):
    """Slaney's scale (librosa's htk=False): 200 / 3 Hz per mel below 1 kHz, ln(6.4) / 27 per mel in log-frequency above"""
    f = np.asarray(f, dtype=np.float64)
    lin = f * 3.0 / 200.0
    log = 15.0 + np.log(np.maximum(f, 1e-300) / 1000.0) * (27.0 / np.log(6.4))
    return np.where(f >= 1000.0, log, lin)


def _mel_to_hz(m):
    m = np.asarray(m, dtype=np.float64)
    return np.where(m >= 15.0, 1000.0 * np.exp((m - 15.0) * (np.log(6.4) / 27.0)), m * 200.0 / 3.0)


def mel_filterbank(sr, n_fft, n_mels):
    """-> fp64 [n_mels, 1 + n_fft // 2]: triangular filters on n_mels + 2 points equally spaced in mel between 0 and sr / 2, evaluated at
    the bin frequencies np.linspace(0, sr / 2, 1 + n_fft // 2), filter m scaled by 2 / (f[m + 2] - f[m]) (Slaney's area normalisation)"""
    bins = np.linspace(0.0, sr / 2.0, 1 + n_fft // 2)
    edges = _mel_to_hz(np.linspace(_hz_to_mel(0.0), _hz_to_mel(sr / 2.0), n_mels + 2))
    width = np.diff(edges)
    ramps = edges[:, None] - bins[None, :]
    rising = -ramps[:-2] / width[:-1, None]
    falling = ramps[2:] / width[1:, None]
    return np.maximum(0.0, np.minimum(rising, falling)) * (2.0 / (edges[2:] - edges[:-2]))[:, None]


def pack_filterbank(fb):
    """the filters as the kernel reads them: (first, ptr, weights) -- filter m owns the bins first[m] .. first[m] + ptr[m + 1] - ptr[m] - 1
    with the fp32 weights[ptr[m] : ptr[m + 1]] (its run from the first to the last non-zero bin)"""
    first, ptr, weights = [], [0], []
    for row in np.asarray(fb, dtype=np.float32):
        nz = np.flatnonzero(row)
        if nz.size == 0:
            raise ValueError('a mel filter is empty: too many bands for this n_fft')
        first.append(int(nz[0]))
        weights.append(row[nz[0]:nz[-1] + 1])
        ptr.append(ptr[-1] + int(nz[-1] - nz[0] + 1))
    return np.asarray(first, dtype=np.int32), np.asarray(ptr, dtype=np.int32), np.concatenate(weights).astype(np.float32)


def mfcc_tables(sr=16000, n_fft=2048, n_mels=128, n_mfcc=50):
    """-> dict of the host tables, built in fp64 and rounded once to fp32 (cached per parameter set): ``window`` [n_fft] periodic Hann;
    ``twiddle`` [n_fft, 2] (cos, -sin)(2 pi m / n_fft); ``mel_first`` / ``mel_ptr`` / ``mel_w`` the packed mel filters; ``dct``
    [n_mfcc, n_mels] the orthonormal DCT-II"""
    key = (int(sr), int(n_fft), int(n_mels), int(n_mfcc))
    if key in _TABLES:
        return _TABLES[key]
    sr, n_fft, n_mels, n_mfcc = key
    if n_fft < 64 or n_fft > 4096 or n_fft & (n_fft - 1):
        raise ValueError(f'n_fft must be a power of two in 64 .. 4096, not {n_fft}')
    if not 1 <= n_mfcc <= n_mels:
        raise ValueError(f'n_mfcc must be in 1 .. n_mels = {n_mels}, not {n_mfcc}')
    phase = 2.0 * np.pi * np.arange(n_fft, dtype=np.float64) / n_fft
    first, ptr, w = pack_filterbank(mel_filterbank(sr, n_fft, n_mels))
    m = np.arange(n_mels, dtype=np.float64)
    dct = np.sqrt(2.0 / n_mels) * np.cos(np.pi * np.arange(n_mfcc, dtype=np.float64)[:, None] * (2.0 * m[None, :] + 1.0) / (2.0 * n_mels))
    dct[0] *= np.sqrt(0.5)
    _TABLES[key] = {'window': (0.5 - 0.5 * np.cos(phase)).astype(np.float32),
                    'twiddle': np.stack([np.cos(phase), -np.sin(phase)], axis=1).astype(np.float32),
                    'mel_first': first, 'mel_ptr': ptr, 'mel_w': w, 'dct': dct.astype(np.float32)}
    return _TABLES[key]


def beta_probs(n_thresholds=100):
    """-> fp64 [n_thresholds]: the mass of Beta(2, 18) between consecutive points of np.linspace(0, 1, n_thresholds + 1), from the closed form
    of its CDF, 1 - (1 - x)^19 - 19 x (1 - x)^18 = 1 - (1 - x)^18 (1 + 18 x) (pYIN's prior over the thresholds).  The polynomial is
    evaluated at the fp64 points in exact rational arithmetic and every mass rounded ONCE: in floating point the difference of two values
    near 1 loses a digit that the 1e-15 agreement with scipy.stats.beta needs."""
    from fractions import Fraction
    x = np.linspace(0.0, 1.0, int(n_thresholds) + 1)
    survival = [(1 - Fraction(float(v))) ** 18 * (1 + 18 * Fraction(float(v))) for v in x]
    return np.array([float(a - b) for a, b in zip(survival[:-1], survival[1:])], dtype=np.float64)


def pyin_tables(sr=16000, fmin=70.0, fmax=500.0, frame_length=2048, win_length=1024, hop=512):
    """-> dict of pYIN's host tables and scalars at librosa 0.8.1's defaults, built in fp64 (cached per parameter set; include/mts.h names
    every entry): ``min_period`` / ``max_period`` / ``n_lags``; ``n_bins`` = floor(120 log2(fmax / fmin)) + 1 pitch bins of a tenth of a
    semitone and ``freqs`` fp32 [n_bins]; ``thresholds`` / ``beta`` [100] and ``beta_head`` [101] (sums of the first m of beta);
    ``boltz_fact`` / ``boltz_exp`` [n_lags // 2 + 2]; ``width`` = 10 round(35.92 * 12 * hop / sr) + 1 and ``ltri`` [width] the log of the
    triangle window; ``lsrc`` [4, n_bins] = log(switch[v][v']) - log(the window's sum inside the bins around j); ``linit`` [2 n_bins];
    ``log_floor`` = log(tiny)"""
    key = ('pyin', int(sr), float(fmin), float(fmax), int(frame_length), int(win_length), int(hop))
    if key in _TABLES:
        return _TABLES[key]
    _, sr, fmin, fmax, frame_length, win_length, hop = key
    if not (0.0 < fmin < fmax <= sr / 2.0):
        raise ValueError(f'pitch: 0 < fmin < fmax <= sr / 2 is expected, not fmin={fmin}, fmax={fmax}')
    min_period = max(int(np.floor(sr / fmax)), 1)
    max_period = min(int(np.ceil(sr / fmin)), frame_length - win_length - 1)
    if max_period < min_period + 2:
        raise ValueError(f'pitch: fmin={fmin}, fmax={fmax} leave fewer than three lags ({min_period} .. {max_period})')
    n_bins = int(np.floor(120.0 * np.log2(fmax / fmin))) + 1
    if 2 * n_bins > 1024:
        raise ValueError(f'pitch: fmin={fmin}, fmax={fmax} give {2 * n_bins} states; 1024 is the most the Viterbi kernel holds')
    n_lags = max_period - min_period + 1
    tiny = np.finfo(np.float64).tiny
    beta = beta_probs(100)
    n_boltz = n_lags // 2 + 2
    count = np.arange(n_boltz, dtype=np.float64)
    fact = np.zeros(n_boltz)
    fact[1:] = (1.0 - np.exp(-2.0)) / (1.0 - np.exp(-2.0 * count[1:]))
    width = 10 * int(round(35.92 * 12.0 * hop / sr)) + 1
    half = width // 2
    tri = 1.0 - np.abs(np.arange(width, dtype=np.float64) - half) / (half + 1.0)
    at = np.arange(n_bins)[:, None] + np.arange(width)[None, :] - half
    norm = np.where((at >= 0) & (at < n_bins), tri[None, :], 0.0).sum(axis=1)
    switch = np.log(np.array([0.99, 0.01, 0.01, 0.99]))
    linit = np.full(2 * n_bins, np.log(tiny))
    linit[n_bins:] = np.log(1.0 / n_bins + tiny)
    _TABLES[key] = {'sr': float(sr), 'fmin': fmin, 'fmax': fmax, 'frame_length': frame_length, 'win_length': win_length, 'hop': hop,
                    'min_period': min_period, 'max_period': max_period, 'n_lags': n_lags, 'n_bins': n_bins, 'bins_per_octave': 120.0,
                    'no_trough_prob': 0.01, 'log_floor': float(np.log(tiny)), 'width': width,
                    'thresholds': np.linspace(0.0, 1.0, 101)[1:].copy(), 'beta': beta,
                    'beta_head': np.array([np.sum(beta[:m]) for m in range(101)]), 'boltz_fact': fact, 'boltz_exp': np.exp(-2.0 * count),
                    'freqs': (fmin * 2.0 ** (np.arange(n_bins, dtype=np.float64) / 120.0)).astype(np.float32), 'ltri': np.log(tri),
                    'lsrc': np.ascontiguousarray(switch[:, None] - np.log(norm)[None, :]), 'linit': linit}
    return _TABLES[key]


def uniform_spans(n_samples, interval=1.0, sr=16000):
    """-> the (start, end) sample spans of the reference's uniform units (extract_embeddings_inference.py:243-247, :406-408), for
    ``ResidentAudio(..., unit='samples')``: ``int((n_samples / sr) // interval)`` units, unit i = [int(sr * interval * i),
    int(sr * (interval * i + 1))).  The window is ONE second whatever the interval: that is what upstream computes."""
    n = int((n_samples / sr) // interval)
    return [(int(sr * (interval * i)), int(sr * (interval * i + 1))) for i in range(n)]


def load_wav(directory, files):
    """-> a list over documents of fp32 waveforms read from ``<directory>/<file>.wav``: 16 kHz mono PCM through scipy.io.wavfile; int16 is
    scaled by 1 / 32768 (int32 by 2^-31, uint8 centred and scaled by 1 / 128, float as it is).  ValueError for another rate or channel
    count: resampling and other containers are the caller's, who can pass arrays to ResidentAudio directly."""
    from scipy.io import wavfile
    out = []
    for name in files:
        path = os.path.join(directory, name if str(name).endswith('.wav') else f'{name}.wav')
        rate, data = wavfile.read(path)
        if rate != 16000:
            raise ValueError(f'load_wav: {path} is sampled at {rate} Hz; 16000 is expected (resample before)')
        if data.ndim != 1:
            raise ValueError(f'load_wav: {path} has {data.shape[1]} channels; mono is expected')
        if data.dtype == np.int16:
            data = data.astype(np.float32) / 32768.0
        elif data.dtype == np.int32:
            data = (data.astype(np.float64) / 2147483648.0).astype(np.float32)
        elif data.dtype == np.uint8:
            data = (data.astype(np.float32) - 128.0) / 128.0
        out.append(np.ascontiguousarray(data, dtype=np.float32))
    return out


class ResidentAudio:
    """The waveforms of a corpus in HBM: ``wave`` fp32 [total_samples] (the documents one after another, ONE upload), ``sent_start`` /
    ``sent_len`` (int64 [total_sentences]: sentence s is the samples sent_start[s] .. sent_start[s] + sent_len[s] of ``wave``).

    ``waves``: a list over documents of 1-d float arrays at ``sr``.  ``spans``: a list over documents of (start, end) per sentence;
    ``unit='seconds'`` converts as the reference does, ``int(sr * t)`` (extract_embeddings.py:108-109, :506-513), ``unit='samples'`` takes
    integers; ``end`` is clipped to the document's length, as the slice ``audio[start:end]`` is.  Sentences may overlap or leave gaps.

    Host tables: ``sentences`` (sentences per document), ``sample_counts`` (samples per sentence), ``frame_counts`` (frames per sentence
    at the default hop of 512: 1 + n // 512), ``n_docs``, ``total_sentences``, ``total_samples``, ``total_frames``, ``nbytes``.  With a
    CPU device only the host tables exist, as for ResidentFrames.

    ValueError, naming the document and the sentence: an empty document, a wave that is not 1-d, a negative start, ``start >= end`` after
    clipping, a sentence shorter than 8 * 512 = 4096 samples.  ValueError for a non-finite sample, found on the device at upload.

    ``min_samples`` (default None: the rule above, which the framed features need) lowers that bound for an audio that feeds
    ``wav2vec2()``, whose shortest sentence is 400 samples: the constructor then refuses only sentences below ``min_samples``, and
    ``mfcc()`` / ``pitch()`` / ``yin()`` / ``prosodic()`` apply the 4096-sample rule when they are called."""

    DEFAULT_HOP = 512

    def __init__(self, waves, spans, device, sr=16000, unit='seconds', min_samples=None):
        if unit not in ('seconds', 'samples'):
            raise ValueError("ResidentAudio: unit must be 'seconds' or 'samples'")
        if min_samples is not None and int(min_samples) < 1:
            raise ValueError(f'ResidentAudio: min_samples must be positive, not {min_samples}')
        self.min_samples = None if min_samples is None else int(min_samples)
        self.sr = int(sr)
        self.device = torch.device(device)
        if self.device.type == 'cuda' and self.device.index is None:
            self.device = torch.device('cuda', torch.cuda.current_device())
        if len(waves) == 0 or len(waves) != len(spans):
            raise ValueError(f'ResidentAudio: {len(waves)} waveforms and {len(spans)} span lists; one list per document and at least one are expected')
        parts, starts, lens, sentences, offset = [], [], [], [], 0
        for d, (w, doc_spans) in enumerate(zip(waves, spans)):
            a = w.detach().cpu().to(torch.float32).numpy() if isinstance(w, torch.Tensor) else np.asarray(w, dtype=np.float32)
            if a.ndim != 1:
                raise ValueError(f'ResidentAudio: the wave of document {d} is {a.ndim}-d; a 1-d array of samples is expected')
            if a.shape[0] == 0:
                raise ValueError(f'ResidentAudio: document {d} has no samples')
            if len(doc_spans) == 0:
                raise ValueError(f'ResidentAudio: document {d} has no sentences')
            for s, (t0, t1) in enumerate(doc_spans):
                b, e = (int(self.sr * t0), int(self.sr * t1)) if unit == 'seconds' else (int(t0), int(t1))
                e = min(e, int(a.shape[0]))
                if b < 0:
                    raise ValueError(f'ResidentAudio: sentence {s} of document {d} starts at sample {b}')
                if b >= e:
                    raise ValueError(f'ResidentAudio: sentence {s} of document {d} is empty: samples {b} .. {e} of {int(a.shape[0])} (start >= end '
                                     'after clipping to the document)')
                if self.min_samples is None:
                    self._refuse_short(e - b, self.DEFAULT_HOP, s, d)
                elif e - b < self.min_samples:
                    raise ValueError(f'ResidentAudio: sentence {s} of document {d} has {e - b} samples, fewer than min_samples = {self.min_samples}')
                starts.append(offset + b)
                lens.append(e - b)
            sentences.append(len(doc_spans))
            parts.append(a)
            offset += int(a.shape[0])
        self.n_docs = len(sentences)
        self.sentences = np.asarray(sentences, dtype=np.int64)
        self.sample_counts = np.asarray(lens, dtype=np.int64)
        self.frame_counts = 1 + self.sample_counts // self.DEFAULT_HOP
        self.total_sentences = int(self.sentences.sum())
        self.total_samples = offset
        self.total_frames = int(self.frame_counts.sum())
        self._start_host = np.asarray(starts, dtype=np.int64)
        self._doc_offset = np.concatenate([[0], np.cumsum([p.shape[0] for p in parts])]).astype(np.int64)
        self.wave = self.sent_start = self.sent_len = None
        self._device_tables = {}
        if self.device.type != 'cuda':
            return
        flat = torch.from_numpy(np.concatenate(parts)) if len(parts) > 1 else torch.from_numpy(np.ascontiguousarray(parts[0]))
        del parts
        self.wave = flat.to(self.device)
        self.sent_start = torch.from_numpy(self._start_host).to(self.device)
        self.sent_len = torch.from_numpy(self.sample_counts).to(self.device)
        self._refuse_non_finite()

    @staticmethod
    def _refuse_short(n, hop, s, d):
        if n < (_DELTA_FRAMES - 1) * hop:
            raise ValueError(f'ResidentAudio: sentence {s} of document {d} has {n} samples, fewer than the {(_DELTA_FRAMES - 1) * hop} that give '
                             f"{_DELTA_FRAMES} frames at a hop of {hop}: librosa's delta needs {_DELTA_FRAMES} frames and the reference raises there")

    def _refuse_short_sentences(self, hop):
        """the constructor's rule for the framed features, applied late to an audio built with ``min_samples``"""
        short = np.flatnonzero(self.sample_counts < (_DELTA_FRAMES - 1) * hop)
        if short.size:
            d, s = self._where(int(short[0]))
            self._refuse_short(int(self.sample_counts[short[0]]), hop, s, d)

    def _where(self, s):
        """flat sentence index -> (document, sentence of the document)"""
        ends = np.cumsum(self.sentences)
        d = int(np.searchsorted(ends, s, side='right'))
        return d, s - (int(ends[d - 1]) if d else 0)

    def _refuse_non_finite(self):
        """one pass over the resident waveform in slices (the check's temporary stays small); the first offender is named"""
        for a in range(0, self.total_samples, _CHECK_SAMPLES):
            ok = torch.isfinite(self.wave[a:a + _CHECK_SAMPLES])
            if not bool(ok.all()):
                i = a + int(torch.nonzero(~ok)[0])
                d = int(np.searchsorted(self._doc_offset, i, side='right')) - 1
                inside = np.flatnonzero((self._start_host <= i) & (i < self._start_host + self.sample_counts))
                where = f' (in sentence {self._where(int(inside[0]))[1]})' if inside.size else ''
                raise ValueError(f'ResidentAudio: sample {i - int(self._doc_offset[d])} of document {d}{where} is not finite (refused here: '
                                 'np.nanmean would skip the frames it spoils)')

    def __len__(self):
        return self.n_docs

    @property
    def nbytes(self):
        """bytes of the resident data (waveform, sentence table, the tables of the parameter sets used so far); 0 on a CPU device"""
        held = [self.wave, self.sent_start, self.sent_len] + [t for tabs in self._device_tables.values() for t in tabs.values()]
        return sum(t.numel() * t.element_size() for t in held if t is not None)

    def _tables(self, n_mfcc, n_mels, n_fft):
        key = (n_mfcc, n_mels, n_fft)
        if key not in self._device_tables:
            host = mfcc_tables(self.sr, n_fft, n_mels, n_mfcc)
            self._device_tables[key] = {k: torch.from_numpy(v).to(self.device) for k, v in host.items()}
        return self._device_tables[key]

    def mfcc(self, n_mfcc=50, n_mels=128, n_fft=2048, hop=512, out_dtype=torch.float32):
        """-> ``frames.ResidentFrames`` on the device: [total_frames, 2 n_mfcc] frames in ``out_dtype`` (torch.float32 | torch.bfloat16; bf16
        is the fp32 value rounded once), columns [0, n_mfcc) the MFCC and [n_mfcc, 2 n_mfcc) its delta, with this audio's sentence table
        (sentence s has 1 + n // hop frames).  Two entry points on the current stream (csrc/mfcc.hip); the mel matrix between them is freed
        before returning.  ValueError: parameters the tables refuse, a sentence shorter than 8 * hop samples (named); RuntimeError on a CPU
        device (there is no CPU fallback)."""
        n_mfcc, n_mels, n_fft, hop = int(n_mfcc), int(n_mels), int(n_fft), int(hop)
        if hop < 1:
            raise ValueError(f'mfcc: hop must be positive, not {hop}')
        if out_dtype not in (torch.float32, torch.bfloat16):
            raise ValueError(f'mfcc: out_dtype is torch.float32 or torch.bfloat16, not {out_dtype}')
        host = mfcc_tables(self.sr, n_fft, n_mels, n_mfcc)
        if hop != self.DEFAULT_HOP or self.min_samples is not None:
            self._refuse_short_sentences(hop)
        if self.device.type != 'cuda':
            raise RuntimeError('ResidentAudio.mfcc runs on the GPU (there is no CPU fallback)')
        del host
        from . import ops
        counts = 1 + self.sample_counts // hop
        start = np.zeros(self.total_sentences + 1, dtype=np.int64)
        np.cumsum(counts, out=start[1:])
        total_frames = int(start[-1])
        with torch.cuda.device(self.device):
            tabs = self._tables(n_mfcc, n_mels, n_fft)
            frame_start = torch.from_numpy(start).to(self.device)
            mel = ops.mel_frames(self.wave, self.sent_start, self.sent_len, frame_start, total_frames, tabs['window'], tabs['twiddle'],
                                 tabs['mel_first'], tabs['mel_ptr'], tabs['mel_w'], hop)
            out = torch.empty((total_frames, 2 * n_mfcc), dtype=out_dtype, device=self.device)
            ops.mfcc_frames(mel, frame_start, tabs['dct'], out)
            del mel
        return ResidentFrames.from_device(out, frame_start, self.sentences)

    def mfcc_stats(self, **kw):
        """-> [total_sentences, 4 n_mfcc] on the device: ``mfcc(**kw).pool('mean_std')``, the reference's ``mfcc`` sentence vector
        [mean x, mean dx, std x, std dx] (200 wide at the defaults)"""
        return self.mfcc(**kw).pool('mean_std')

    # ---- prosodic features (csrc/prosody.hip) ----------------------------------------------------------------------------------------
    PROSODIC_WIDTH = 167
    PITCH_WORKSPACE = 1 << 30                  # bytes of cmnd / shift / log-observations / backpointers a chunk of sentences may take

    def _frame_start_host(self):
        start = np.zeros(self.total_sentences + 1, dtype=np.int64)
        np.cumsum(self.frame_counts, out=start[1:])
        return start

    def _pitch_tables(self, fmin, fmax):
        """pyin_tables with its arrays on the device (cached); ValueError for parameters the tables refuse"""
        host = pyin_tables(self.sr, fmin, fmax)
        if self.device.type != 'cuda':
            return host
        key = ('pyin', float(fmin), float(fmax))
        if key not in self._device_tables:
            self._device_tables[key] = {k: torch.from_numpy(v).to(self.device) for k, v in host.items() if isinstance(v, np.ndarray)}
        return {**host, **self._device_tables[key]}

    def _pitch_pass(self, who, fmin, fmax, pyin, yin, trough_threshold=0.1, workspace_bytes=None):
        """the frame-level tracks of the whole corpus, sentence chunk by sentence chunk: the per-frame temporaries (cmnd and shift, and for
        pYIN the fp64 log-observations and the int16 backpointers: 8.4 KB per frame at the defaults) exist for one chunk at a time, sized
        to ``workspace_bytes`` -- never for the corpus.  -> dict of device tensors [total_frames]"""
        tabs = self._pitch_tables(fmin, fmax)
        if not 0.0 < float(trough_threshold):
            raise ValueError(f'{who}: trough_threshold must be positive, not {trough_threshold}')
        if self.device.type != 'cuda':
            raise RuntimeError(f'ResidentAudio.{who} runs on the GPU (there is no CPU fallback)')
        self._refuse_short_sentences(self.DEFAULT_HOP)
        from . import ops
        start = self._frame_start_host()
        n_lags, S = tabs['n_lags'], 2 * tabs['n_bins']
        per_frame = 8 * n_lags + (10 * S if pyin else 0)
        budget = max(int(workspace_bytes if workspace_bytes is not None else self.PITCH_WORKSPACE) // per_frame, 1)
        out = {}
        with torch.cuda.device(self.device):
            new = lambda dtype: torch.empty(self.total_frames, dtype=dtype, device=self.device)
            if pyin:
                out.update(f0=new(torch.float32), voiced_prob=new(torch.float32), voiced=new(torch.uint8))
            if yin:
                out['yin_f0'] = new(torch.float32)
            a = 0
            while a < self.total_sentences:
                b = max(int(np.searchsorted(start, start[a] + budget, side='right')) - 1, a + 1)
                fa, fb = int(start[a]), int(start[b])
                local = torch.from_numpy(start[a:b + 1] - start[a]).to(self.device)
                cmnd, shift = ops.yin_frames(self.wave, self.sent_start[a:b], self.sent_len[a:b], local, fb - fa, tabs['min_period'],
                                             tabs['max_period'], tabs['frame_length'], tabs['win_length'], tabs['hop'])
                if pyin:
                    _, logobs = ops.pyin_observe(cmnd, shift, tabs, voiced_prob=out['voiced_prob'][fa:fb])
                    ops.pyin_viterbi(logobs, local, tabs, f0=out['f0'][fa:fb], voiced=out['voiced'][fa:fb])
                    del logobs
                if yin:
                    ops.yin_pick(cmnd, shift, tabs['min_period'], self.sr, trough_threshold, f0=out['yin_f0'][fa:fb])
                del cmnd, shift
                a = b
        return out

    def pitch(self, fmin=70.0, fmax=500.0, workspace_bytes=None):
        """-> (f0, voiced_prob, voiced) on the device, [total_frames] each (frames of 2048 every 512 samples, sentence s owns the frames
        ``frame_counts[:s].sum()`` onwards): pYIN as librosa 0.8.1 defines it -- ``f0`` fp32, NaN where unvoiced; ``voiced_prob`` fp32;
        ``voiced`` bool.  ValueError for fmin / fmax the tables refuse; RuntimeError on a CPU device."""
        r = self._pitch_pass('pitch', fmin, fmax, True, False, workspace_bytes=workspace_bytes)
        return r['f0'], r['voiced_prob'], r['voiced'].view(torch.bool)

    def yin(self, fmin=70.0, fmax=500.0, trough_threshold=0.1):
        """-> the plain-YIN f0 per frame, fp32 [total_frames] on the device (``librosa.yin(y, fmin, fmax)``: the first trough of the
        normalised difference function below ``trough_threshold``, else its global minimum)"""
        return self._pitch_pass('yin', fmin, fmax, False, True, trough_threshold=trough_threshold)['yin_f0']

    def prosodic(self, out_dtype=torch.float32, out=None, workspace_bytes=None):
        """-> [total_sentences, 167] on the device in ``out_dtype`` (torch.float32 | torch.bfloat16: ONE rounding of the fp32 row), the
        reference's ``prosodic`` sentence vector in its column order: [f0 mean, f0 std, pause mean, pause std, voiced-intensity mean,
        voiced-intensity std, mel mean (40), mel std (40), delta-mel mean (40), delta-mel std (40), pitch_jump].  ``out``: a [total_sentences,
        167] fp32 / bf16 view with unit column stride (a column block of a wider matrix: nothing outside it is written) to fill instead.
        pitch_jump is 0 on the first sentence of every document.  RuntimeError on a CPU device."""
        if out is None and out_dtype not in (torch.float32, torch.bfloat16):
            raise ValueError(f'prosodic: out_dtype is torch.float32 or torch.bfloat16, not {out_dtype}')
        if out is not None and (out.dim() != 2 or tuple(out.shape) != (self.total_sentences, self.PROSODIC_WIDTH) or out.stride(1) != 1
                                or out.dtype not in (torch.float32, torch.bfloat16)):
            raise ValueError(f'prosodic: out must be a fp32 / bf16 [{self.total_sentences}, {self.PROSODIC_WIDTH}] view with unit column stride')
        if self.device.type != 'cuda':
            raise RuntimeError('ResidentAudio.prosodic runs on the GPU (there is no CPU fallback)')
        from . import ops
        tracks = self._pitch_pass('prosodic', 70.0, 500.0, True, True, workspace_bytes=workspace_bytes)
        first = np.zeros(self.total_sentences, dtype=np.uint8)
        first[np.concatenate([[0], np.cumsum(self.sentences)[:-1]])] = 1
        with torch.cuda.device(self.device):
            if out is None:
                out = torch.empty((self.total_sentences, self.PROSODIC_WIDTH), dtype=out_dtype, device=self.device)
            tabs = self._tables(1, 40, 2048)
            frame_start = torch.from_numpy(self._frame_start_host()).to(self.device)
            mel = ops.mel_frames(self.wave, self.sent_start, self.sent_len, frame_start, self.total_frames, tabs['window'], tabs['twiddle'],
                                 tabs['mel_first'], tabs['mel_ptr'], tabs['mel_w'], self.DEFAULT_HOP)
            ops.frame_pool(mel, frame_start, out[:, 6:86], first='mean', with_std=True)
            delta = ops.frame_delta(mel, frame_start)
            del mel
            ops.frame_pool(delta, frame_start, out[:, 86:166], first='mean', with_std=True)
            del delta
            ops.prosodic_stats(tracks['f0'], tracks['voiced_prob'], tracks['yin_f0'], frame_start, torch.from_numpy(first).to(self.device),
                               out, self.PROSODIC_WIDTH - 1)
        return out

    # ---- wav2vec 2.0 frames (csrc/wav2vec2.hip, wav2vec2.py) -------------------------------------------------------------------------
    W2V_WORKSPACE = 1 << 30                    # bytes of activations a chunk of sentences may take
    W2V_STATS_MODES = ('mean', 'max', 'mean_std', 'max_std', 'last')

    def _w2v_chunks(self, who, weights, out_dtype, workspace_bytes):
        """the checks of the two wav2vec 2.0 passes and the chunking -> (frame_start [total_sentences + 1], [(a, b)]): sentences a .. b - 1
        go through the encoder together; a chunk's activations stay within ``workspace_bytes`` (one sentence at the least) and within the
        32-bit row indexing of the attention kernels"""
        from . import wav2vec2 as W
        if not isinstance(weights, W.Wav2Vec2Weights):
            raise ValueError(f'{who}: weights must be a Wav2Vec2Weights (Wav2Vec2Weights.from_state_dict)')
        if out_dtype not in (torch.float32, torch.bfloat16):
            raise ValueError(f'{who}: out_dtype is torch.float32 or torch.bfloat16, not {out_dtype}')
        frames = W.frame_counts(self.sample_counts, weights.kernels, weights.strides)
        short = np.flatnonzero(frames < 1)
        if short.size:
            d, s = self._where(int(short[0]))
            raise ValueError(f'ResidentAudio: sentence {s} of document {d} has {int(self.sample_counts[short[0]])} samples, fewer than the '
                             f"{weights.min_samples} that give one wav2vec 2.0 frame: upstream's Conv1d raises there")
        if self.device.type != 'cuda':
            raise RuntimeError(f'ResidentAudio.{who} runs on the GPU (there is no CPU fallback)')
        if weights.device != self.device:
            raise ValueError(f'{who}: the weights live on {weights.device}, the audio on {self.device}')
        start = np.zeros(self.total_sentences + 1, dtype=np.int64)
        np.cumsum(frames, out=start[1:])
        cost = W.chunk_bytes(weights, self.sample_counts)
        budget = int(workspace_bytes if workspace_bytes is not None else self.W2V_WORKSPACE)
        rows_cap = ((1 << 31) - 1) // (3 * weights.hidden_size)        # n_sent * longest sentence of a chunk: what mts_full_attn_fwd indexes
        chunks, a = [], 0
        while a < self.total_sentences:
            b, used, longest = a, 0, 0
            while b < self.total_sentences:
                longest_b = max(longest, int(frames[b]))
                if b > a and (used + int(cost[b]) > budget or (b - a + 1) * longest_b > rows_cap):
                    break
                used, longest, b = used + int(cost[b]), longest_b, b + 1
            chunks.append((a, b))
            a = b
        return start, chunks

    def _w2v_pass(self, weights, start, chunks, emit, pos='auto'):
        from . import wav2vec2 as W
        with torch.cuda.device(self.device):
            for a, b in chunks:
                plan = W.ChunkPlan(self.sample_counts[a:b], weights, self.device)
                emit(a, b, plan, lambda out: W.forward_chunk(weights, self.wave, self.sent_start[a:b], self.sent_len[a:b], plan, out, pos=pos))

    def wav2vec2(self, weights, out_dtype=torch.float32, workspace_bytes=None, out=None, pos='auto'):
        """-> ``frames.ResidentFrames`` of width ``weights.hidden_size`` on the device: ``Wav2Vec2Model(...).last_hidden_state`` of every
        sentence, each normalised to zero mean and unit variance and encoded as a sequence of its own (wav2vec2.py).  Sentence s owns
        T_s rows, T <- (T - k) // stride + 1 through the conv layers of its n samples (49 for 16 000 at the base configuration).  The
        frames are made a chunk of sentences at a time: a chunk's activations (3 200 x 512 values per second of audio for the first
        conv layer alone) stay within ``workspace_bytes`` (default 1 GiB), only the [total_frames, H] result is kept.  ``out``: a
        contiguous [total_frames, H] fp32 / bf16 device matrix to fill instead of a new one of ``out_dtype``.  ``pos``: the positional
        convolution's form, 'kernel' | 'gemm' | 'auto'.  ValueError, naming the document and the sentence, for a sentence that gives no
        frame (upstream's Conv1d raises there); RuntimeError on a CPU device."""
        start, chunks = self._w2v_chunks('wav2vec2', weights, out.dtype if out is not None else out_dtype, workspace_bytes)
        total, H = int(start[-1]), weights.hidden_size
        if out is None:
            out = torch.empty((total, H), dtype=out_dtype, device=self.device)
        elif tuple(out.shape) != (total, H) or not out.is_contiguous() or out.device != self.device:
            raise ValueError(f'wav2vec2: out must be a contiguous [{total}, {H}] matrix on {self.device}')
        self._w2v_pass(weights, start, chunks, lambda a, b, plan, run: run(out[int(start[a]):int(start[b])]), pos=pos)
        return ResidentFrames.from_device(out, torch.from_numpy(start).to(self.device), self.sentences)

    def wav2vec2_stats(self, weights, mode='mean_std', out_dtype=torch.float32, workspace_bytes=None, pos='auto'):
        """-> [total_sentences, W] on the device: ``wav2vec2(weights).pool(mode)`` without keeping the frames -- every chunk is pooled into
        its rows of the result and freed.  Modes: 'mean', 'max', 'mean_std', 'max_std', 'last'.  'delta_gap' reads the NEXT sentence's
        first frame, which another chunk may hold: pool the frames instead, ``wav2vec2(weights).pool('delta_gap')``."""
        if mode == 'delta_gap':
            raise ValueError("wav2vec2_stats: 'delta_gap' reads the next sentence's first frame, which another chunk may hold; keep the frames: "
                             "audio.wav2vec2(weights).pool('delta_gap')")
        if mode not in self.W2V_STATS_MODES:
            raise ValueError(f'wav2vec2_stats: mode is one of {self.W2V_STATS_MODES}, not {mode!r}')
        start, chunks = self._w2v_chunks('wav2vec2_stats', weights, out_dtype, workspace_bytes)
        from . import ops
        H = weights.hidden_size
        width = 2 * H if mode.endswith('_std') else H
        pooled = torch.empty((self.total_sentences, width), dtype=out_dtype, device=self.device)

        def emit(a, b, plan, run):
            frames = run(torch.empty((plan.total_frames, H), dtype=out_dtype, device=self.device))
            if mode == 'last':
                ops.frame_edges(frames, plan.dev['frame_start'], None, pooled[a:b], 'last')
            else:
                ops.frame_pool(frames, plan.dev['frame_start'], pooled[a:b], first=mode.split('_')[0], with_std=mode.endswith('_std'))

        self._w2v_pass(weights, start, chunks, emit, pos=pos)
        return pooled
