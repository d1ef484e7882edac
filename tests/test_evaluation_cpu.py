"""evaluation.summarize (pure numpy) on a hand-built table, and the binding of cofi_eval_monitors."""
import numpy as np
import pytest

from cofii2p_amd import _lib, evaluation, metrics


def hand_table(thr):
    """five frames: three solved, one failed pose (NaN errors), one without matches (NaN mean residual, zero counts, failed pose)"""
    T = len(thr)
    rows = np.zeros((5, 6 + T))
    n = [40, 10, 7, 0, 25]
    success = [1, 1, 0, 0, 1]
    rte = [0.5, 7.0, np.nan, np.nan, 2.0]
    rre = [1.5, 3.0, np.nan, np.nan, 12.0]
    rmse = [2.5, 4.0, 9.0, np.nan, 1.0]
    rng = np.random.default_rng(3)
    for f in range(5):
        rows[f, :6] = [n[f], success[f], max(0, n[f] - 2) if success[f] else 0, rte[f], rre[f], rmse[f]]
        if n[f]:
            res = rng.uniform(0, 12, n[f])
            rows[f, 6:] = (res[None, :] <= thr[:, None]).sum(1)
    return rows, n, success, rte, rre, rmse


@pytest.mark.parametrize("thr", [None, np.array([5.0, 1.0, 2.5])])
def test_summarize_on_a_hand_built_table(thr):
    t = metrics.pixel_thresholds() if thr is None else thr
    rows, n, success, rte, rre, rmse = hand_table(t)
    s = evaluation.summarize(rows, thr)
    assert s["n"].tolist() == n and s["success"].tolist() == [bool(v) for v in success]
    np.testing.assert_array_equal(s["rte"], rte)
    np.testing.assert_array_equal(s["rre"], rre)
    np.testing.assert_array_equal(s["rmse"], rmse)
    # the error arrays eval_all.py:138-139 saves: successful frames only, in frame order
    np.testing.assert_array_equal(s["t_error"], [0.5, 7.0, 2.0])
    np.testing.assert_array_equal(s["r_error"], [1.5, 3.0, 12.0])
    assert s["report"] == metrics.report(np.array([1.5, 3.0, 12.0]), np.array([0.5, 7.0, 2.0]))
    rec = metrics.registration_recall(s["r_error"], s["t_error"], 10, 5)
    assert rec["num_success"] == 1 and rec["num_frames"] == 3 and rec["r_mean"] == 1.5
    assert "\n".join(metrics.report_lines(rec)) in "\n".join(s["report"])
    # ir = count / n per frame; ir_curve = its mean over the frames that have matches (IR_RMSE.py:68)
    assert s["ir"].shape == (5, len(t)) and np.all(np.isnan(s["ir"][3]))
    have = [0, 1, 2, 4]
    for f in have:
        np.testing.assert_array_equal(s["ir"][f], rows[f, 6:] / n[f])
    np.testing.assert_array_equal(s["ir_curve"], np.stack([rows[f, 6:] / n[f] for f in have]).mean(0))
    assert s["frames_without_matches"].tolist() == [3]
    np.testing.assert_array_equal(s["thresholds"], t)


def test_summarize_edge_cases():
    thr = np.array([1.0, 2.0])
    none = np.array([[0, 0, 0, np.nan, np.nan, np.nan, 0, 0]] * 2, dtype=np.float64)   # no frame has matches, no pose succeeded
    s = evaluation.summarize(none, thr)
    assert np.all(np.isnan(s["ir_curve"])) and s["t_error"].shape == (0,) and s["frames_without_matches"].tolist() == [0, 1]
    assert s["report"] == metrics.report(np.zeros(0), np.zeros(0))
    with pytest.raises(ValueError):
        evaluation.summarize(np.zeros((3, 7)), thr)                      # 6 + T columns
    unwritten = np.full((2, 8), np.nan)
    with pytest.raises(ValueError):
        evaluation.summarize(unwritten, thr)                             # a row no frame wrote


def test_binding_and_header():
    names = set(_lib.header_symbols())
    assert "cofi_eval_monitors" in names
    res, args = _lib.SIGNATURES["cofi_eval_monitors"]
    assert res is _lib.c_int and len(args) == 20
    assert _lib.ABI_VERSION == 3                                          # an additive change
    with pytest.raises(_lib.CofiError):
        evaluation.EvalTable(4, device="cpu")                             # there is no CPU path
