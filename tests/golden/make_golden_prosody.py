#!/usr/bin/env python3
"""Generate g24_pauses.npz by running the REFERENCE's get_pause_durations (extract_acoustic_features.py:20-55) itself.

Run in the build container only (needs the reference checkout, MTS_REFERENCE or /root/reference, which never travels to the GPU box):

    python tests/golden/make_golden_prosody.py

The function is pure Python; its module imports ``librosa`` at the top, which is not installed, so an empty placeholder module stands in
for it (nothing of it is called).  Only inputs and the reference's outputs are stored -- never reference source.  The fixture is data:
``values`` fp32 (the intensity vectors one after another), ``offsets`` int64 [n + 1], and per vector the returned pause lengths
(``pauses`` / ``pause_offsets``) and voiced values (``voiced`` fp64 / ``voiced_offsets``).
"""
import os
import sys
import types

import numpy as np

REF = os.environ.get('MTS_REFERENCE', '/root/reference')
OUT = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, REF)
sys.modules.setdefault('librosa', types.ModuleType('librosa'))

from extract_acoustic_features import get_pause_durations  # noqa: E402


def vectors():
    rng = np.random.default_rng(24)
    v = [np.full(9, 0.9), np.full(9, 0.1), np.full(1, 0.7), np.full(1, 0.2),                        # all voiced, all pause, one frame
         np.r_[np.full(6, 0.8), np.full(4, 0.1)], np.r_[np.full(3, 0.0), np.full(7, 0.6)],          # a trailing pause only, a leading pause
         np.r_[0.8, 0.1, 0.1, 0.9, 0.2, 0.2, 0.2], np.r_[0.1, 0.9, 0.1, 0.1, 0.9, 0.1],              # closed and then an open run
         np.tile([0.9, 0.1], 6), np.tile([0.1, 0.9], 6),                                             # alternating frames
         np.full(8, 0.5), np.r_[0.5, 0.4999999, 0.5, 0.5000001, 0.0, 0.5], np.r_[0.0, 0.5],          # exactly 0.5 is voiced
         np.r_[np.full(5, 0.49), 0.5], np.r_[0.5, np.full(5, 0.49)], np.zeros(12), np.ones(12),
         np.r_[1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 1.0, 0.0, 0.0, 1.0]]
    for n in (9, 10, 17, 24, 24, 33, 64, 65, 100, 129, 200):                                        # random tracks, two of them sticky
        v.append(rng.random(n))
        v.append(np.repeat(rng.random((n + 3) // 4), 4)[:n])
    return [np.asarray(a, dtype=np.float32) for a in v]


def main():
    vs = vectors()
    pauses, voiced = [], []
    for a in vs:
        p, s = get_pause_durations(a)
        pauses.append(np.asarray(p, dtype=np.int64))
        voiced.append(np.asarray(s, dtype=np.float64))
    off = lambda parts: np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.int64)
    np.savez(os.path.join(OUT, 'g24_pauses.npz'), values=np.concatenate(vs), offsets=off(vs), pauses=np.concatenate(pauses),
             pause_offsets=off(pauses), voiced=np.concatenate(voiced), voiced_offsets=off(voiced))
    print(f'wrote g24_pauses.npz: {len(vs)} vectors')


if __name__ == '__main__':
    main()
