"""CPU-only: the test pass's public surface -- exports, signatures and defaults, the saturated-logit form of a hypothesis without a
threshold, and the refusals that need no GPU."""
import inspect

import numpy as np
import pytest


def test_exports():
    import multimodaltopicsegmentation_amd as pkg
    from multimodaltopicsegmentation_amd import evaluate as module_or_function
    from multimodaltopicsegmentation_amd.trainer import NativeTrainer
    for name in ('evaluate', 'bootstrap_ci', 'paired_bootstrap', 'cross_validate'):
        assert name in pkg.__all__ and callable(getattr(pkg, name)), name
    assert callable(module_or_function)                                   # the package attribute is the function, as `fit`
    assert callable(NativeTrainer.evaluate) and 'evaluate.evaluate' in NativeTrainer.evaluate.__doc__
    from multimodaltopicsegmentation_amd import ops
    assert callable(ops.bootstrap_sums)


def test_signatures_and_defaults():
    from multimodaltopicsegmentation_amd import bootstrap_ci, cross_validate, evaluate, paired_bootstrap
    p = inspect.signature(evaluate).parameters
    assert list(p)[:2] == ['trainer_or_model', 'corpus']
    want = {'batch_size': 8, 'threshold': None, 'end_boundary': False, 'winpr_k': 10, 'zero_baseline': False, 'return_scores': False}
    assert {k: p[k].default for k in want} == want and all(p[k].kind is inspect.Parameter.KEYWORD_ONLY for k in want)
    assert 'metric' not in p                                                # metric 'b' is not offered at all
    for fn in (bootstrap_ci, paired_bootstrap):
        q = inspect.signature(fn).parameters
        assert (q['samples'].default, q['seed'].default, q['device'].default) == (10000, 0, None)
    assert list(inspect.signature(cross_validate).parameters)[:2] == ['make_trainer', 'folds']
    with pytest.raises(ValueError):
        cross_validate(lambda: None, [])


def test_saturated_logits_decide_as_the_tags_at_one_half():
    from multimodaltopicsegmentation_amd.evaluate import SATURATED, _saturated
    tags = [[0, 1, 1, 0], [1], []]
    h = _saturated(tags, 5, 'cpu')
    assert tuple(h.shape) == (3, 5, 1) and h.dtype.is_floating_point and h.element_size() == 4
    prob = 1.0 / (1.0 + np.exp(-h.numpy()[..., 0].astype(np.float64)))
    want = np.zeros((3, 5), dtype=bool)
    want[0, 1:3] = True
    want[1, 0] = True
    assert np.array_equal(prob > 0.5, want) and np.array_equal(np.abs(h.numpy()), np.full((3, 5, 1), SATURATED, dtype=np.float32))


def test_an_empty_corpus_is_refused_before_any_device_work():
    from multimodaltopicsegmentation_amd import evaluate

    class Empty:
        def __len__(self):
            return 0
    with pytest.raises(ValueError, match='no documents'):
        evaluate(object(), Empty())
