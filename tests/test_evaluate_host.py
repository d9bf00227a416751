"""CPU: the host side of held-out pair validation -- metrics from counts, the threshold set, the reference's LossHistory files,
and the new entry points' argument checks (no device work)."""
import os

import numpy as np
import pytest


def test_metrics_from_counts():
    from deepmerge_amd.evaluate import PairEvalResult
    # 10 pairs, 4 positive; at the margin (1.0): 3 positives and 1 negative merged
    r = PairEvalResult.from_counts(10, 4, 2.5, 1.0, [0.5, 1.0, 2.0], [1, 3, 4], [0, 1, 6])
    assert (r.n_pairs, r.n_pos, r.n_neg, r.loss) == (10, 4, 6, 0.25)
    assert (r.tp, r.fp, r.fn, r.tn) == (3, 1, 1, 5)
    assert r.precision == 3 / 4 and r.recall == 3 / 4 and r.f_score == 0.75 and r.accuracy == 0.8
    assert r.thresholds == (0.5, 1.0, 2.0) and r.merged_pos == (1, 3, 4) and r.merged_neg == (0, 1, 6)
    assert r.best_threshold == 1.0 and r.best_f_score == 0.75


def test_zero_denominators_give_zero():
    from deepmerge_amd.evaluate import PairEvalResult, prf
    assert prf(0, 0, 0) == (0.0, 0.0, 0.0)
    assert prf(0, 5, 0) == (0.0, 0.0, 0.0)
    assert prf(0, 0, 5) == (0.0, 0.0, 0.0)
    r = PairEvalResult.from_counts(3, 0, 0.0, 1.0, [1.0], [0], [0])           # no positive pair at all, nothing merged
    assert (r.precision, r.recall, r.f_score, r.accuracy) == (0.0, 0.0, 0.0, 1.0)
    assert r.best_threshold == 1.0 and r.best_f_score == 0.0


def test_best_threshold_takes_the_smallest_of_equal_f():
    from deepmerge_amd.evaluate import PairEvalResult
    # F at the four thresholds: 0, 2/3, 2/3, 0.5 -> the first of the two maxima
    r = PairEvalResult.from_counts(8, 2, 0.0, 0.3, [0.1, 0.2, 0.3, 0.4], [0, 1, 2, 2], [0, 0, 2, 6])
    fs = [0.0, 2 / 3, 2 * 0.5 * 1.0 / 1.5, 2 * 0.25 * 1.0 / 1.25]
    assert fs[1] == fs[2]
    assert r.best_f_score == fs[1] and r.best_threshold == float(np.float32(0.2))
    assert r.f_score == fs[2]


def test_result_needs_the_margin_among_its_thresholds():
    from deepmerge_amd.evaluate import PairEvalResult
    with pytest.raises(ValueError, match="margin"):
        PairEvalResult.from_counts(4, 2, 0.0, 1.0, [0.5], [1], [1])


def test_threshold_set_merges_the_margin():
    from deepmerge_amd.evaluate import default_thresholds, threshold_set
    t = threshold_set([0.25, 0.5, 2.0], 1.0)
    assert t.dtype == np.float32 and t.tolist() == [0.25, 0.5, 1.0, 2.0]
    assert threshold_set([0.5, 1.0], 1.0).tolist() == [0.5, 1.0]               # already there: no duplicate
    assert threshold_set([3.0], 1.0).tolist() == [1.0, 3.0]
    d = threshold_set(None, 1.5)
    assert np.array_equal(d, default_thresholds(1.5)) and np.float32(1.5) in d and len(d) == 64
    assert len(threshold_set(np.arange(1, 1024, dtype=np.float32), 0.5)) == 1024


@pytest.mark.parametrize("bad, match", [([0.5, float("nan")], "finite"), ([float("inf")], "finite"), ([1e39], "finite"),
                                        ([0.5, 0.5], "ascending"), ([0.7, 0.6], "ascending"), ([], "at least one"),
                                        (np.arange(1, 1025, dtype=np.float32) + 0.5, "at most 1024")])
def test_threshold_set_refuses(bad, match):
    from deepmerge_amd.evaluate import threshold_set
    with pytest.raises(ValueError, match=match):
        threshold_set(bad, 1.0)


def test_evaluator_refuses_bad_thresholds_before_device_work():
    """The threshold checks run before anything touches the model or the dataset."""
    from deepmerge_amd.evaluate import PairEvaluator

    class Untouchable:
        def __getattr__(self, name):
            raise AssertionError(f"touched .{name}")

    for bad in ([], [1.0, float("nan")], [2.0, 1.0], list(range(1, 1026))):
        with pytest.raises(ValueError):
            PairEvaluator(Untouchable(), Untouchable(), thresholds=bad)
    with pytest.raises(ValueError, match="batch"):
        PairEvaluator(Untouchable(), Untouchable(), batch=0)


def test_loss_history_writes_the_reference_layout(tmp_path):
    from deepmerge_amd.callbacks import LossHistory
    h = LossHistory(str(tmp_path))
    assert os.path.dirname(h.save_path) == str(tmp_path) and os.path.basename(h.save_path) == "loss_" + h.time_str
    assert len(h.time_str.split("_")) == 6
    h.append_loss(0.5, 0.25, 0.75)
    h.append_loss(0.4, 0.3, 12.34)
    for kind, want in (("loss", ["0.5", "0.4"]), ("val_loss", ["0.25", "0.3"]), ("f_score", ["0.75", "12.34"])):
        path = os.path.join(h.save_path, f"epoch_{kind}_{h.time_str}.txt")
        with open(path) as f:
            assert f.read() == "".join(v + "\n" for v in want)
    assert (h.losses, h.val_loss, h.f_scores) == ([0.5, 0.4], [0.25, 0.3], [0.75, 12.34])
    txt = sorted(f for f in os.listdir(h.save_path) if f.endswith(".txt"))
    assert txt == sorted(f"epoch_{k}_{h.time_str}.txt" for k in ("loss", "val_loss", "f_score"))


def test_train_refuses_the_training_set_as_validation_set():
    from deepmerge_amd import Train_SMT
    ds = object()
    with pytest.raises(ValueError, match="val_dataset"):
        Train_SMT.train(None, 1.0, 4, 1e-4, 0.0, 0.0, 0.1, 0, dataset=ds, val_dataset=ds)


def test_library_checks_eval_arguments_before_any_launch():
    import __graft_entry__ as g
    from deepmerge_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        g.build()
    lib = _lib.lib()
    assert lib.dm_contrastive_terms(1, 1, 1, 1.0, 1, 1, 0, 8, None) == -1
    assert lib.dm_contrastive_terms(1, 1, 1, 1.0, 1, 1, 4, 0, None) == -1
    assert lib.dm_pair_eval_summary(1, 1, 1, 0, 1, 4, 1, 1, 1, 1, None) == -1
    assert lib.dm_pair_eval_summary(1, 1, 1, 2 ** 31, 1, 4, 1, 1, 1, 1, None) == -1
    assert lib.dm_pair_eval_summary(1, 1, 1, 10, 1, 0, 1, 1, 1, 1, None) == -6
    assert lib.dm_pair_eval_summary(1, 1, 1, 10, 1, 1025, 1, 1, 1, 1, None) == -6
    assert b"thresholds" in lib.dm_last_error()
    assert lib.dm_pair_eval_workspace_bytes(10 ** 6, 1024) == 8 * 2 * 1025 + 8 * 245
    assert lib.dm_pair_eval_workspace_bytes(0, 4) == 0
