#!/usr/bin/env python3
"""Generate g23_segment_audio.npz: the sample spans of the reference's ``BasePredictor.segment_audio`` (predict.py:92-129), recorded from
the reference's own method through its ``mock_audio`` path, on the CPU.

Run in the build container only (needs the reference checkout, which never travels to the GPU box):

    python tests/golden/make_golden_segment_audio.py

The reference's predict.py imports packages that are not installed here (librosa, pytorch_lightning, scipy.io.wavfile) and modules of
its own that pull in more.  None of them is touched by ``segment_audio`` when ``mock_audio`` is given at the predictor's own sample rate,
so every import other than numpy and torch is stubbed in ``sys.modules`` (an empty module with a ``__spec__`` and the imported names set
to None) before ``import predict``.  A bare ``BasePredictor`` then gets the three attributes the method reads (``sr``, ``interval``,
``adapt``).

Stored per case i: ``n{i}`` (samples), ``sr{i}``, ``interval{i}`` (float64, as a user passes it), ``adaptive{i}``, ``flags{i}`` (int64,
one per basic unit), ``raises{i}`` (1 when the reference raised IndexError) and ``spans{i}`` (int64 [k, 2]; empty when it raised).
Data only; no reference source.
"""
import importlib.machinery
import os
import sys
import types

import numpy as np

REF = os.environ.get('MTS_REFERENCE', '/root/reference')
OUT = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True

STUBS = {'librosa': (), 'pytorch_lightning': ('Trainer',), 'scipy': (), 'scipy.io': (), 'scipy.io.wavfile': ('write',),
         'EncoderDataset': ('AudioPortionDatasetInference',), 'models': (), 'models.lightning_model': ('TextSegmenter',), 'utils': (),
         'utils.load_datasets_precomputed': ('load_dataset_for_inference',), 'extract_embeddings_inference': ('main',)}

# (samples, sr, interval, adaptive, flags)
CASES = [
    (41, 4, 1, False, [0, 1, 0, 0, 1, 0, 0, 0, 0, 1]),              # the tail (40, 41)
    (40, 4, 1, False, [0, 1, 0, 0, 1, 0, 0, 0, 0, 1]),              # ends ON a boundary: the empty span (40, 40) is appended all the same
    (41, 4, 1, False, [1, 0, 1]),                                   # the flags run out: the walk stops, the tail spans the rest
    (41, 4, 1, False, [0, 1] * 10),                                 # more flags than units
    (41, 4, 2.7, False, [1, 1, 0, 1, 0]),                           # int(interval) = 2
    (41, 4, 1, False, [0] * 10),                                    # no boundary: one span
    (3, 4, 1, False, [1]),                                          # shorter than one unit
    (1000, 16, 1, True, [int(k % 7 == 3) for k in range(100)]),     # adaptive: 100 units of 10 samples, no tail appended
    (1000, 16, 1, True, [1] * 100),
    (1099, 16, 1, True, [int(k % 5 == 0) for k in range(120)]),     # 10 does not divide 1099: 109 units walked, 120 flags suffice
    (1050, 16, 1, True, [int(k % 9 == 1) for k in range(100)]),     # 105 units walked with 100 flags: IndexError
    (150, 16, 1, True, [0] * 100),                                  # units of 1 sample: IndexError at the 101st
]


def stub_imports():
    for name, attrs in STUBS.items():
        mod = types.ModuleType(name)
        mod.__spec__ = importlib.machinery.ModuleSpec(name, None)
        if '.' not in name:
            mod.__path__ = []
        for a in attrs:
            setattr(mod, a, None)
        sys.modules[name] = mod
    for name in STUBS:
        if '.' in name:
            parent, child = name.rsplit('.', 1)
            setattr(sys.modules[parent], child, sys.modules[name])


def main():
    stub_imports()
    sys.path.insert(0, REF)
    import predict as upstream
    out = {'cases': np.array(len(CASES), dtype=np.int64)}
    for i, (n, sr, interval, adaptive, flags) in enumerate(CASES):
        p = upstream.BasePredictor()
        p.sr, p.interval, p.adapt = sr, interval, adaptive
        raised = 0
        try:
            spans, audio = p.segment_audio(None, list(flags), mock_audio=np.zeros(n, dtype=np.float32), mock_sr=sr)
            assert len(audio) == n
        except IndexError:
            spans, raised = [], 1
        out[f'n{i}'], out[f'sr{i}'] = np.array(n, dtype=np.int64), np.array(sr, dtype=np.int64)
        out[f'interval{i}'], out[f'adaptive{i}'] = np.array(interval, dtype=np.float64), np.array(int(adaptive), dtype=np.int64)
        out[f'flags{i}'], out[f'raises{i}'] = np.array(flags, dtype=np.int64), np.array(raised, dtype=np.int64)
        out[f'spans{i}'] = np.array(spans, dtype=np.int64).reshape(-1, 2)
        print(i, n, sr, interval, adaptive, 'IndexError' if raised else spans)
    assert out['spans0'].tolist() == [[0, 8], [8, 20], [20, 40], [40, 41]]
    assert out['spans1'].tolist()[-1] == [40, 40] and out['raises10'] == 1 and out['raises11'] == 1 and out['raises9'] == 0
    path = os.path.join(OUT, 'g23_segment_audio.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
