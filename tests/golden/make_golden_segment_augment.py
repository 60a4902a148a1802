#!/usr/bin/env python3
"""Generate g22_segment_augment.npz: the reference's segment-order augmentation, run by the reference itself on the CPU.

Run in the build container only (needs the reference checkout, which never travels to the GPU box):

    python tests/golden/make_golden_segment_augment.py

``cross_validation_split(dataset, num_folds, n_test_folds, inverse_augmentation=True)`` (utils/load_datasets_precomputed.py:56-100) is
imported as it stands -- the module needs nothing but numpy and torch -- and called on seven synthetic documents of width D = 3 with seven
folds.  The last fold tests on the seventh document and trains on the first six, so its training list is those six followed by what the
augmentation appended.  The upstream loop runs on into its own appended entries until it has looked at 11 list entries (:74-78), so the
list ends up 17 long; the six entries behind the originals are the originals' twins, which is all the fixture keeps.

Stored per document i: ``emb{i}`` [n, 3] float32 and ``lab{i}`` [n] int64 (inputs), ``twin_emb{i}`` and ``twin_lab{i}`` (the reference's
appended entry; an EMPTY float tensor of shape [0] and an empty label list for a document without a boundary, :92-96), and ``train_len``,
the length of the training list after the call.  Data only; no reference source.
"""
import os
import sys

import numpy as np
import torch

REF = os.environ.get('MTS_REFERENCE', '/root/reference')
OUT = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, REF)

from utils.load_datasets_precomputed import cross_validation_split  # noqa: E402

# a one-row document; no boundary; every row but the last a boundary; two ordinary ones (the loader forces the last label to 0, :172);
# one that ends ON a boundary (no tail: only a hand-made list can hold it)
LABELS = [[0], [0, 0, 0, 0], [1, 1, 1, 1, 0], [0, 0, 1, 0, 1, 0, 0], [0, 1, 0, 0, 0, 1, 1, 0, 0], [0, 1, 0, 1]]
D = 3


def main():
    rng = np.random.default_rng(2222)
    docs = [(torch.from_numpy(rng.standard_normal((len(y), D)).astype(np.float32)), list(y)) for y in LABELS]
    held_out = (torch.zeros(2, D), [0, 0])
    n = len(docs)
    folds = cross_validation_split(docs + [held_out], num_folds=n + 1, n_test_folds=1, inverse_augmentation=True)
    assert len(folds) == n + 1
    train, test = folds[n]
    assert len(test) == 1 and test[0] is held_out and all(train[i] is docs[i] for i in range(n))
    assert len(train) == n + 11, len(train)                      # the loop looked at 11 entries, its own twins among them
    out = {'train_len': np.array(len(train), dtype=np.int64)}
    for i, (emb, lab) in enumerate(docs):
        twin_emb, twin_lab = train[n + i]
        out[f'emb{i}'], out[f'lab{i}'] = emb.numpy().copy(), np.array(lab, dtype=np.int64)
        out[f'twin_emb{i}'], out[f'twin_lab{i}'] = twin_emb.numpy().astype(np.float32), np.array(twin_lab, dtype=np.int64)
        if 1 not in lab:
            assert twin_emb.numel() == 0 and twin_lab == []      # a document without a boundary: an empty twin
        else:
            assert twin_emb.shape == (max(k for k, v in enumerate(lab) if v) + 1, D) and twin_lab[-1] == 1
    path = os.path.join(OUT, 'g22_segment_augment.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
