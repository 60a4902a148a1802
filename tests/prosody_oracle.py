"""NumPy restatement of the reference's ``prosodic`` sentence encoder (extract_acoustic_features.py:20-55, :74-108 on librosa 0.8.1's
``pyin`` / ``yin`` defaults), for the tests only.  Written from the definition in include/mts.h, not from
multimodaltopicsegmentation_amd/audio.py: neither imports the other, and tests/test_prosody_cpu.py compares their tables.  fp64 is the
checker; ``cmnd_shift(y, np.float32)`` keeps the difference function, its running mean and the shifts in single precision with NumPy's
own summation order, and its error against the fp64 run on the same input is the yardstick of tests/test_gpu_prosody.py.

Per sentence y (sr = 16000): frames of 2048 every 512 samples as for MFCC (tests/mfcc_oracle.py); d(tau) = sum_{j=1..1024} (x[j] -
x[j + tau])^2 for tau = 1 .. max_period (the DIRECT form); cmnd = d / (running mean of d + tiny); parabolic shifts; pYIN's observation model
(100 thresholds, Beta(2, 18) prior, Boltzmann(2) prior over the troughs below a threshold, 0.01 for the lowest trough where none is) over
pitch bins of a tenth of a semitone; a DENSE fp64 Viterbi over 2 n_bins states; plain YIN; the pause statistics of get_pause_durations;
mean and std of the 40-band mel power and of its delta; the pitch jump against the previous sentence's plain-YIN track."""
import functools
import math

import numpy as np

from tests import mfcc_oracle as MO

SR, FRAME, WIN, HOP = 16000, 2048, 1024, 512
TINY32 = float(np.finfo(np.float32).tiny)
TINY = float(np.finfo(np.float64).tiny)


# ---- tables ------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def tables(fmin=70.0, fmax=500.0, sr=SR):
    from scipy.signal import get_window
    from scipy.stats import beta as beta_dist
    t = {}
    t['min_period'] = max(int(math.floor(sr / fmax)), 1)
    t['max_period'] = min(int(math.ceil(sr / fmin)), FRAME - WIN - 1)
    t['n_lags'] = t['max_period'] - t['min_period'] + 1
    nb = t['n_bins'] = int(math.floor(12 * 10 * math.log2(fmax / fmin))) + 1
    t['fmin'], t['sr'] = fmin, sr
    t['thresholds'] = np.linspace(0, 1, 101)[1:]
    # the mass of every interval: from the CDF in the lower half, from the survival function above it -- near 1 the CDF's differences are
    # rounding noise of 1e-16 where the true masses are far smaller, and a trough below the last thresholds only takes exactly those
    edges = np.linspace(0, 1, 101)
    t['beta'] = np.where(edges[1:] <= 0.5, np.diff(beta_dist.cdf(edges, 2, 18)), -np.diff(beta_dist.sf(edges, 2, 18)))
    t['freqs'] = fmin * 2.0 ** (np.arange(nb) / 120.0)
    width = t['width'] = int(round(35.92 * 12 * HOP / sr)) * 10 + 1
    half = width // 2
    window = get_window('triangle', width, fftbins=False)
    # transition_local(n_bins, width, window='triangle', wrap=False): row i is the window centred on i, cut at the ends, normalised
    local = np.zeros((nb, nb))
    for i in range(nb):
        for k in range(width):
            j = i + k - half
            if 0 <= j < nb:
                local[i, j] = window[k]
    norm = local.sum(axis=1)
    t['ltri'] = np.log(window)
    switch = np.array([[0.99, 0.01], [0.01, 0.99]])
    t['lsrc'] = np.stack([np.log(switch[v, w]) - np.log(norm) for v in range(2) for w in range(2)])
    p_init = np.zeros(2 * nb)
    p_init[nb:] = 1.0 / nb
    t['linit'] = np.log(p_init + TINY)
    t['log_floor'] = math.log(TINY)
    t['local'] = local / norm[:, None]
    for v in t.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return t


# ---- the difference function ---------------------------------------------------------------------------------------------------------------
def cmnd_shift(y, dtype=np.float64, fmin=70.0, fmax=500.0):
    """one sentence -> (cmnd, shift) [T, n_lags] in ``dtype``"""
    t = tables(fmin, fmax)
    lo, hi = t['min_period'], t['max_period']
    x = MO.frame_signal(np.asarray(y, dtype=dtype), FRAME, HOP)
    d = np.empty((x.shape[0], hi + 1), dtype=dtype)
    d[:, 0] = 0
    for tau in range(1, hi + 1):
        e = x[:, 1:WIN + 1] - x[:, 1 + tau:WIN + 1 + tau]
        d[:, tau] = (e * e).sum(axis=1)
    mean = np.cumsum(d[:, 1:], axis=1) / np.arange(1, hi + 1, dtype=dtype)[None, :]
    c = d[:, lo:hi + 1] / (mean[:, lo - 1:hi] + dtype(TINY32))
    a = (c[:, :-2] + c[:, 2:] - dtype(2) * c[:, 1:-1]) / dtype(2)
    b = (c[:, 2:] - c[:, :-2]) / dtype(2)
    sh = np.zeros_like(c)
    with np.errstate(divide='ignore', invalid='ignore'):
        sh[:, 1:-1] = -b / (dtype(2) * a + dtype(TINY32))
    sh[~(np.abs(sh) <= 1)] = 0
    assert c.dtype == dtype and sh.dtype == dtype
    return c, sh


def troughs(c):
    """c [n_lags] -> bool [n_lags]"""
    out = np.zeros(c.shape[0], dtype=bool)
    out[1:-1] = (c[1:-1] < c[:-2]) & (c[1:-1] <= c[2:])
    out[-1] = c[-1] < c[-2]
    out[0] = c[0] < c[1]
    return out


# ---- pYIN's observation model ----------------------------------------------------------------------------------------------------------------
def observe(c, sh, fmin=70.0, fmax=500.0):
    """cmnd, shift of ONE frame (any float dtype; taken as they are) -> (voiced_prob fp64, obs fp64 [n_bins] the voiced bins' mass)"""
    t = tables(fmin, fmax)
    nb = t['n_bins']
    obs = np.zeros(nb)
    idx = np.flatnonzero(troughs(c))
    if idx.size == 0:
        return 0.0, obs
    h = c[idx].astype(np.float64)
    below = h[:, None] < t['thresholds'][None, :]
    pos = np.cumsum(below, axis=0) - 1
    count = below.sum(axis=0)
    with np.errstate(divide='ignore', invalid='ignore'):
        prior = (1.0 - math.exp(-2.0)) / (1.0 - np.exp(-2.0 * count))[None, :] * np.exp(-2.0 * pos)
    prior[~below] = 0.0
    probs = np.zeros(idx.size)
    for k in range(100):            # one chain in ascending threshold order
        probs = probs + prior[:, k] * t['beta'][k]
    lowest = int(np.argmin(h))
    probs[lowest] += 0.01 * np.sum(t['beta'][:int((~below[lowest]).sum())])
    period = (t['min_period'] + idx).astype(np.float64) + sh[idx].astype(np.float64)
    with np.errstate(divide='ignore', invalid='ignore'):
        bins = np.round(120.0 * np.log2((t['sr'] / period) / fmin))
    bins = np.clip(np.where(np.isnan(bins), 0, bins), 0, nb).astype(int)
    full = np.zeros(nb + 1)
    full[bins] = probs              # the last of equal bins wins; bin nb is dropped
    obs[:] = full[:nb]
    return float(np.clip(obs.sum(), 0.0, 1.0)), obs


def log_observations(vp, obs):
    """-> fp64 [2 n_bins]"""
    nb = obs.shape[0]
    return np.concatenate([np.log(obs + TINY), np.full(nb, math.log((1.0 - vp) / nb + TINY))])


# ---- the Viterbi, dense --------------------------------------------------------------------------------------------------------------------
def viterbi(logobs, ltri, lsrc, linit, log_floor):
    """logobs fp64 [T, 2 n_bins] of ONE sentence and the tables -> states int [T].  Every frame builds the whole [source, target] matrix:
    fl(fl(value[j] + lsrc[2 v + v'][j]) + ltri[.]) inside the band, fl(value[j] + log_floor) outside it, and np.argmax takes the first of
    equals."""
    T, S = logobs.shape
    nb, half = S // 2, ltri.shape[0] // 2
    off = np.arange(nb)[None, :] - np.arange(nb)[:, None]            # target - source
    band = np.abs(off) <= half
    tri = np.where(band, ltri[np.clip(off + half, 0, 2 * half)], 0.0)
    value = logobs[0] + linit
    ptr = np.zeros((T, S), dtype=np.int64)
    for t in range(1, T):
        cand = np.empty((S, S))
        for v in range(2):
            src_val = value[v * nb:(v + 1) * nb]
            for w in range(2):
                inside = (src_val + lsrc[2 * v + w])[:, None] + tri
                cand[v * nb:(v + 1) * nb, w * nb:(w + 1) * nb] = np.where(band, inside, (src_val + log_floor)[:, None])
        ptr[t] = np.argmax(cand, axis=0)
        value = logobs[t] + cand[ptr[t], np.arange(S)]
    states = np.empty(T, dtype=np.int64)
    states[-1] = int(np.argmax(value))
    for t in range(T - 1, 0, -1):
        states[t - 1] = ptr[t, states[t]]
    return states


def track(states, freqs):
    """-> (f0 fp64 with NaN where unvoiced, voiced bool)"""
    nb = freqs.shape[0]
    voiced = states < nb
    return np.where(voiced, freqs[states % nb], np.nan), voiced


def pyin(y, fmin=70.0, fmax=500.0):
    """one sentence, all fp64 -> (f0, voiced_prob, voiced)"""
    t = tables(fmin, fmax)
    c, sh = cmnd_shift(y, np.float64, fmin, fmax)
    rows = [observe(c[i], sh[i], fmin, fmax) for i in range(c.shape[0])]
    lo = np.stack([log_observations(vp, obs) for vp, obs in rows])
    f0, voiced = track(viterbi(lo, t['ltri'], t['lsrc'], t['linit'], t['log_floor']), t['freqs'])
    return f0, np.array([vp for vp, _ in rows]), voiced


# ---- plain YIN -----------------------------------------------------------------------------------------------------------------------------
def yin_pick(c, sh, min_period, sr=SR, threshold=0.1):
    """cmnd, shift [T, n_lags] (fp32 as the device holds them, or fp64) -> f0 [T] in their dtype"""
    dtype = c.dtype.type
    out = np.empty(c.shape[0], dtype=c.dtype)
    for i in range(c.shape[0]):
        ok = troughs(c[i]) & (c[i] < dtype(threshold))
        lag = int(np.argmax(ok)) if ok.any() else int(np.argmin(c[i]))
        with np.errstate(divide='ignore'):
            out[i] = dtype(sr) / (dtype(min_period + lag) + sh[i, lag])
    return out


def yin(y, fmin=70.0, fmax=500.0):
    c, sh = cmnd_shift(y, np.float64, fmin, fmax)
    return yin_pick(c, sh, tables(fmin, fmax)['min_period'])


# ---- the sentence statistics ---------------------------------------------------------------------------------------------------------------
def pauses(intensity, delta=0.5):
    """-> (pause lengths, voiced intensities): a pause is a run of frames below ``delta`` that a frame at or above it CLOSES; a run still
    open at the end is dropped -- unless nothing was closed: then the lists are ([that run], the voiced values and a 0) or, without any
    pause frame, ([0], every intensity)"""
    lengths, kept, run = [], [], 0
    for v in intensity:
        if v < delta:
            run += 1
        else:
            if run:
                lengths.append(run)
                run = 0
            kept.append(v)
    if not lengths:
        if run:
            return np.array([run]), np.array(kept + [0])
        return np.array([0]), np.asarray(intensity)
    return np.array(lengths), np.array(kept)


def scalar_stats(f0, vp, prev, first):
    """f0 (NaN where unvoiced), voiced_prob, the previous sentence's plain-YIN track (None or ``first``: no previous sentence) ->
    fp64 [7]: the six scalar columns and pitch_jump"""
    f0 = np.asarray(f0, dtype=np.float64).copy()
    if np.isnan(f0).all():
        f0[:] = 0.0
    lengths, kept = pauses(np.asarray(vp))
    out = [np.nanmean(f0), np.nanstd(f0), lengths.mean(), lengths.std(), np.mean(kept, dtype=np.float64), np.std(kept, dtype=np.float64)]
    jump = 0.0
    if prev is not None and not first:
        prev = np.asarray(prev, dtype=np.float64)
        with np.errstate(all='ignore'):
            import warnings
            with warnings.catch_warnings():
                warnings.simplefilter('ignore')
                jump = np.nanmean(f0[:len(f0) // 5] / np.nanmean(f0)) - np.nanmean(prev[-len(prev) // 5:] / np.nanmean(prev))
        if np.isnan(jump):
            jump = 0.0
    return np.array(out + [jump])


def mel40(y, dtype=np.float64):
    return MO.mel_power(y, dtype, n_mels=40)


def row_from_tracks(f0, vp, prev, first, mel):
    """-> fp64 [167] from one sentence's tracks and its mel power [T, 40]"""
    s = scalar_stats(f0, vp, prev, first)
    d = MO.delta(mel)
    return np.concatenate([s[:6], mel.mean(axis=0), mel.std(axis=0), d.mean(axis=0), d.std(axis=0), s[6:]])


def prosodic_row(y, prev_y=None):
    """one sentence (and the previous one of its document) -> fp64 [167]"""
    f0, vp, _ = pyin(y)
    return row_from_tracks(f0, vp, None if prev_y is None else yin(prev_y), prev_y is None, mel40(y))


# ---- the test corpus -----------------------------------------------------------------------------------------------------------------------
def _voice(rng, n, f_a, f_b, noise):
    """a harmonic glide from f_a to f_b with a little noise"""
    f = np.linspace(f_a, f_b, n)
    phase = 2 * np.pi * np.cumsum(f) / SR
    return sum(np.sin(k * phase) / k for k in (1, 2, 3)) * 0.3 + noise * rng.standard_normal(n)


@functools.lru_cache(maxsize=None)
def corpus():
    """-> (waves, spans, names): two documents of fp32 samples, 13 sentences of 4096 .. 12 000 samples (9 .. 24 frames) at odd offsets.
    Voiced glides and noise; 'silent' is exact zeros (no voiced frame: the NaN -> 0 rows), 'gap' has a pause inside, 'tail' ends in
    silence (an unclosed pause only), 'noise' is unvoiced noise."""
    rng = np.random.default_rng(20241021)
    kinds = [[('v4096', 4096), ('v12000', 12000), ('gap', 9000), ('silent', 5000), ('after', 6001), ('tail', 8000), ('noise', 7000)],
             [('d1first', 4607), ('d1v', 10001), ('d1low', 8191), ('d1high', 8192), ('d1gap2', 11999), ('d1last', 4608)]]
    waves, spans, names = [], [], []
    for doc in kinds:
        parts, sp, at = [np.zeros(3)], [], 3
        for i, (name, n) in enumerate(doc):
            fa, fb = rng.uniform(90, 220), rng.uniform(90, 320)
            w = _voice(rng, n, fa, fb, 0.01)
            if name == 'silent':
                w[:] = 0.0
            elif name in ('gap', 'd1gap2'):
                w[n // 3:n // 3 + 3000] = 0.0
                if name == 'd1gap2':
                    w[8000:10500] = 0.0
            elif name == 'tail':
                w[5000:] = 0.0
            elif name == 'noise':
                w = 0.2 * rng.standard_normal(n)
            elif name == 'd1low':
                w = _voice(rng, n, 75.0, 80.0, 0.0)
            elif name == 'd1high':
                w = _voice(rng, n, 480.0, 440.0, 0.0)
            parts.append(w)
            sp.append((at, at + n))
            names.append(name)
            at += n
        wave = np.concatenate(parts).astype(np.float32)
        wave.setflags(write=False)
        waves.append(wave)
        spans.append(tuple(sp))
    return tuple(waves), tuple(spans), tuple(names)


def sentences():
    """-> [(name, fp32 samples, index of its document, first of the document)]"""
    waves, spans, names = corpus()
    out, k = [], 0
    for d, (w, doc) in enumerate(zip(waves, spans)):
        for i, (a, b) in enumerate(doc):
            out.append((names[k], w[a:b], d, i == 0))
            k += 1
    return out


@functools.lru_cache(maxsize=None)
def reference_cmnd(dtype_name, fmin=70.0, fmax=500.0):
    """-> per sentence (cmnd, shift) in 'float64' or 'float32', computed once (read-only)"""
    dtype = {'float64': np.float64, 'float32': np.float32}[dtype_name]
    out = []
    for _, y, _, _ in sentences():
        c, sh = cmnd_shift(y, dtype, fmin, fmax)
        c.setflags(write=False)
        sh.setflags(write=False)
        out.append((c, sh))
    return tuple(out)
