"""The evaluation pass on the device: cofi_eval_monitors (csrc/evaluation.hip), evaluation.eval_monitors / EvalTable / evaluate, the
eval_into tail of forward_async and FrameBatcher(eval_table=...).

Yardsticks: the reference's own record (tests/golden/metrics.npz, evaluation/IR_RMSE.py on five result files), cofii2p_amd.metrics in
float64 (the host restatement of that script) and pose.pose_errors (the same device function: bit-equal).  The synthetic operand tests
use cap = 96, B = 6 and counts (96, 37, 4, 3, 0, 64): a full buffer, a partial last wave, the PnP minimum, a count below it, an empty frame
and an exact wave, in capacity-sized buffers with finite junk beyond count."""
import os

import numpy as np
import pytest
import torch
from scipy.spatial.transform import Rotation

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CAP = 96
COUNTS = (96, 37, 4, 3, 0, 64)
SUCCESS = (1, 1, 1, 0, 0, 1)
GOLD = os.path.join(os.path.dirname(__file__), "golden", "metrics.npz")


@pytest.fixture(scope="module")
def ev():
    from cofii2p_amd import evaluation
    return evaluation


def bits(t):
    """float64 tensor / array -> its bit patterns (NaN-safe equality)"""
    a = t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def frame_K(f):
    return np.array([[700.0 + 12.5 * f, 0, 256.0 + f], [0, 690.0 + 8.0 * f, 80.0 - 0.5 * f], [0, 0, 1.0]], dtype=np.float32)


def synth_batch(seed):
    """host arrays of one batch: X (B,CAP,3), uv (B,CAP,2) float32, K (B,3,3) float32, P_gt (B,4,4) float64 holding float32 values (so a float32
    copy is the same matrix), pose (B,12) float32 near the ground truth, result (B,3) int32"""
    rng = np.random.default_rng(seed)
    B = len(COUNTS)
    X = rng.uniform(-20, 20, (B, CAP, 3)).astype(np.float32)
    X[:, :, 2] = rng.uniform(-5, 5, (B, CAP)).astype(np.float32)
    uv = np.zeros((B, CAP, 2), np.float32)
    Ks = np.stack([frame_K(f) for f in range(B)])
    P = np.zeros((B, 4, 4))
    pose = np.zeros((B, 12), np.float32)
    for f in range(B):
        R = Rotation.from_rotvec(rng.normal(size=3) * 0.4).as_matrix()
        t = rng.normal(size=3) * 2 + np.array([0, 0, 30.0])
        P[f] = np.eye(4)
        P[f, :3, :3], P[f, :3, 3] = R, t
        P[f] = P[f].astype(np.float32).astype(np.float64)
        cam = X[f].astype(np.float64) @ P[f, :3, :3].T + P[f, :3, 3]
        proj = cam @ Ks[f].astype(np.float64).T
        uv[f] = (proj[:, :2] / proj[:, 2:] + rng.normal(size=(CAP, 2)) * 3.0).astype(np.float32)   # residuals spread over the 0 .. 10 px thresholds
        Rp = Rotation.from_rotvec(rng.normal(size=3) * 0.02).as_matrix() @ R
        pose[f, :9], pose[f, 9:] = Rp.reshape(9), t + rng.normal(size=3) * 0.1
    result = np.array([[SUCCESS[f], max(0, COUNTS[f] - 1), f] for f in range(B)], np.int32)
    return X, uv, Ks, P, pose, result


def reference_rows(X, uv, Ks, P, counts, thr):
    """(n, rmse, ir (B,T), residuals) per frame from cofii2p_amd.metrics on float64 casts; a frame without matches: NaN, zeros"""
    from cofii2p_amd import metrics
    out = []
    for f, n in enumerate(counts):
        if n == 0:
            out.append((0, np.nan, np.zeros(len(thr)), np.zeros(0)))
            continue
        xy = uv[f, :n].T.astype(np.float64)
        ir, rmse = metrics.inlier_ratio_rmse(xy, X[f, :n].astype(np.float64), P[f].astype(np.float64), Ks[f].astype(np.float64), thr)
        res = np.sum(np.square(xy - metrics.gt_pixels(X[f, :n].astype(np.float64), P[f].astype(np.float64), Ks[f].astype(np.float64))), axis=0) ** 0.5
        out.append((n, rmse, ir, res))
    return out


@pytest.fixture(scope="module")
def batch():
    """the synthetic batch (first seed whose float64 residuals keep 1e-9 px from every threshold; at most one seed is passed over), its
    float64 reference computed once, and the device operands"""
    from cofii2p_amd import metrics
    thr = metrics.pixel_thresholds()
    for seed in (40, 41):
        host = synth_batch(seed)
        ref = reference_rows(host[0], host[1], host[2], host[3], COUNTS, thr)
        gap = min(np.abs(r[3][None, :] - thr[:, None]).min() for r in ref if r[0])
        if gap > 1e-9:
            break
    else:
        raise AssertionError("two seeds in a row with a residual within 1e-9 px of a threshold")
    X, uv, Ks, P, pose, result = host
    d = {"host": host, "ref": ref, "thr": thr, "seed": seed,
         "X": torch.from_numpy(X).to(DEV), "uv": torch.from_numpy(uv).to(DEV), "K": torch.from_numpy(Ks).to(DEV),
         "P": torch.from_numpy(P).to(DEV), "pose": torch.from_numpy(pose).to(DEV), "result": torch.from_numpy(result).to(DEV),
         "count": torch.tensor(COUNTS, dtype=torch.int32, device=DEV)}
    return d


def run(ev, b, rows=None, row_index=None, frames=None, **over):
    """one launch on (a subset of) the batch -> the table's rows on the host"""
    sel = slice(None) if frames is None else torch.tensor(frames, device=DEV)
    g = lambda k: over[k] if k in over else (b[k] if frames is None else b[k][sel].contiguous())
    n = len(COUNTS) if frames is None else len(frames)
    table = ev.EvalTable(rows or n, device=DEV)
    ops = {"object_points": g("X"), "image_points": g("uv"), "count": g("count"), "pose": g("pose"), "result": g("result"),
           "coord_major": over.get("coord_major", False)}
    ev.eval_monitors(ops, g("K"), g("P"), table, row_index)
    return table.host()


# ------------------------------------------------------------------------------------------------ 1. the reference's record
def test_against_the_reference_record(ev):
    from cofii2p_amd import metrics
    gold = np.load(GOLD, allow_pickle=False)
    nf = len(gold["frame_order"])
    fr = [{k: gold["f%d_%s" % (i, k)] for k in ("GT_P", "pred_P", "K", "fine_xy", "object_points")} for i in range(nf)]
    ns = [f["fine_xy"].shape[1] for f in fr]
    assert ns == [37, 4, 258, 120, 61]
    cap = max(ns)
    X = np.full((nf, cap, 3), 7.0, np.float32)
    xy = np.full((nf, 2, cap), 3.0, np.float32)
    pose = np.zeros((nf, 12), np.float32)
    for i, f in enumerate(fr):
        assert f["fine_xy"].dtype == f["object_points"].dtype == f["GT_P"].dtype == f["K"].dtype == np.float32 and f["pred_P"].dtype == np.float64
        X[i, :ns[i]], xy[i, :, :ns[i]] = f["object_points"], f["fine_xy"]
        pose[i, :9], pose[i, 9:] = f["pred_P"][:3, :3].reshape(9), f["pred_P"][:3, 3]
    table = ev.EvalTable(nf, device=DEV)
    ops = {"object_points": torch.from_numpy(X).to(DEV), "image_points": torch.from_numpy(xy).to(DEV), "coord_major": True,
           "count": torch.tensor(ns, dtype=torch.int32, device=DEV), "pose": torch.from_numpy(pose).to(DEV),
           "result": torch.tensor([[1, n, 0] for n in ns], dtype=torch.int32, device=DEV)}
    ev.eval_monitors(ops, np.stack([f["K"] for f in fr]), torch.from_numpy(np.stack([f["GT_P"] for f in fr])), table)   # one launch; float32 P_gt
    rows = table.host()
    irs = []
    for i, f in enumerate(fr):
        ir, _ = metrics.inlier_ratio_rmse(f["fine_xy"], f["object_points"], f["GT_P"], f["K"])   # the script's own dtypes
        got = rows[i, 6:] / rows[i, 0]
        assert rows[i, 0] == ns[i]
        np.testing.assert_array_equal(got, ir)
        irs.append(got)
        rec = float(gold["rmse"][0, list(gold["frame_order"]).index(i)])
        print("frame %d: mean residual %.9f, recorded %.9f, |d| %.3e" % (i, rows[i, 5], rec, abs(rows[i, 5] - rec)))
        assert abs(rows[i, 5] - rec) <= 1e-5
    assert np.abs(np.mean(irs, 0) - gold["ir"]).max() <= 1e-12
    s = ev.summarize(rows)
    assert np.abs(s["ir_curve"] - gold["ir"]).max() <= 1e-12


# ------------------------------------------------------------------------------------------------ 2. numpy in float64
def test_against_numpy_float64(ev, batch):
    from cofii2p_amd import pose as pose_mod
    rows = run(ev, batch)
    assert rows.shape == (6, 6 + 51) and batch["seed"] in (40, 41)
    want_err = pose_mod.pose_errors(batch["pose"], batch["P"]).cpu().numpy()
    for f, (n, rmse, ir, _res) in enumerate(batch["ref"]):
        assert rows[f, 0] == n and rows[f, 1] == SUCCESS[f] and rows[f, 2] == max(0, n - 1)
        if n:
            np.testing.assert_array_equal(rows[f, 6:] / n, ir)
            rel = abs(rows[f, 5] - rmse) / abs(rmse)
            print("frame %d (n = %d): mean residual relative difference %.3e" % (f, n, rel))
            assert rel <= 1e-10
        else:
            assert np.isnan(rows[f, 5]) and np.all(rows[f, 6:] == 0)
        if SUCCESS[f]:
            assert np.array_equal(bits(rows[f, 3:5]), bits(want_err[f])) and np.all(np.isfinite(rows[f, 3:5]))
        else:
            assert np.isnan(rows[f, 3]) and np.isnan(rows[f, 4])
    assert rows[0, 6:].max() > 0 and rows[0, 6:].min() < COUNTS[0]   # the thresholds really split the residuals


# ------------------------------------------------------------------------------------------------ 3. operands in place
def test_operands_in_place(ev, batch):
    base = run(ev, batch)
    c2 = torch.full((len(COUNTS), 2), -7, dtype=torch.int32, device=DEV)   # the forward's (B, 2) count tensor
    c2[:, 0] = batch["count"]
    assert c2[:, 0].stride(0) == 2
    np.testing.assert_array_equal(bits(run(ev, batch, count=c2[:, 0])), bits(base))
    np.testing.assert_array_equal(bits(run(ev, batch, uv=batch["uv"].transpose(1, 2).contiguous(), coord_major=True)), bits(base))
    np.testing.assert_array_equal(bits(run(ev, batch, P=batch["P"].to(torch.float32))), bits(base))
    # a negative count is an empty frame
    neg = batch["count"].clone()
    neg[1] = -3
    r = run(ev, batch, count=neg)
    assert r[1, 0] == 0 and np.isnan(r[1, 5]) and np.all(r[1, 6:] == 0)
    np.testing.assert_array_equal(bits(r[[0, 2, 3, 4, 5]]), bits(base[[0, 2, 3, 4, 5]]))
    # count=None: every row of every frame is read
    full = run(ev, batch, count=torch.full((len(COUNTS),), CAP, dtype=torch.int32, device=DEV))
    none = run(ev, batch, count=None)
    np.testing.assert_array_equal(bits(none), bits(full))
    assert np.all(none[:, 0] == CAP)
    np.testing.assert_array_equal(bits(none[0]), bits(base[0]))           # the full frame is the full frame
    assert not np.array_equal(bits(none[1, 5:]), bits(base[1, 5:]))        # the rows beyond count were read


# ------------------------------------------------------------------------------------------------ 4. independence
def test_frames_are_independent(ev, batch):
    base = run(ev, batch)
    for f in range(len(COUNTS)):
        np.testing.assert_array_equal(bits(run(ev, batch, frames=[f])[0]), bits(base[f]))
    perm = [4, 2, 0, 5, 1, 3]
    p = run(ev, batch, frames=perm)
    for pos, f in enumerate(perm):
        np.testing.assert_array_equal(bits(p[pos]), bits(base[f]))


# ------------------------------------------------------------------------------------------------ 5. row_index
def test_row_index(ev, batch):
    base = run(ev, batch)
    idx = [7, 0, 9, 3, 4, 1]
    got = run(ev, batch, rows=10, row_index=torch.tensor(idx, dtype=torch.int32, device=DEV))
    for f, r in enumerate(idx):
        np.testing.assert_array_equal(bits(got[r]), bits(base[f]))
    for r in set(range(10)) - set(idx):
        assert np.all(np.isnan(got[r]))
    # -1 for two frames: sentinel-filled rows stay as they are, and so does every other row nobody was sent to
    table = ev.EvalTable(10, device=DEV)
    table.rows.fill_(-12345.0)
    idx = [7, -1, 9, -1, 4, 1]
    ops = {"object_points": batch["X"], "image_points": batch["uv"], "count": batch["count"], "pose": batch["pose"], "result": batch["result"]}
    ev.eval_monitors(ops, batch["K"], batch["P"], table, idx)   # a host list is uploaded
    got = table.host()
    for f, r in enumerate(idx):
        if r >= 0:
            np.testing.assert_array_equal(bits(got[r]), bits(base[f]))
    for r in set(range(10)) - {r for r in idx if r >= 0}:
        assert np.all(got[r] == -12345.0), r
    # an index beyond the table writes nothing either
    table.rows.fill_(-1.0)
    ev.eval_monitors(ops, batch["K"], batch["P"], table, [10, 11, 1 << 30, 0, -5, 12])
    got = table.host()
    np.testing.assert_array_equal(bits(got[0]), bits(base[3]))
    assert np.all(got[1:] == -1.0)


# ------------------------------------------------------------------------------------------------ 6. capture
def test_call_is_capturable(ev, batch):
    """record, overwrite the inputs in place with another batch, replay once: the rows of the eager call on the new inputs"""
    X2, uv2, K2, P2, pose2, res2 = (torch.from_numpy(a).to(DEV) for a in synth_batch(77))
    cnt2 = torch.tensor([90, 30, 5, 4, 1, 0], dtype=torch.int32, device=DEV)
    X, uv, K, P, pose, res, cnt = (batch[k].clone() for k in ("X", "uv", "K", "P", "pose", "result", "count"))
    ri = torch.arange(6, dtype=torch.int32, device=DEV)
    table = ev.EvalTable(6, device=DEV)
    ops = {"object_points": X, "image_points": uv, "count": cnt, "pose": pose, "result": res}
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):   # warm-up outside the capture: code objects are loaded
        ev.eval_monitors(ops, K, P, table, ri)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ev.eval_monitors(ops, K, P, table, ri)
    X.copy_(X2), uv.copy_(uv2), K.copy_(K2), P.copy_(P2), pose.copy_(pose2), res.copy_(res2), cnt.copy_(cnt2)
    table.rows.fill_(float("nan"))
    g.replay()
    torch.cuda.synchronize()
    got = table.host()
    t2 = ev.EvalTable(6, device=DEV)
    ev.eval_monitors({"object_points": X2, "image_points": uv2, "count": cnt2, "pose": pose2, "result": res2}, K2, P2, t2, ri)
    want = t2.host()
    np.testing.assert_array_equal(bits(got), bits(want))
    assert want[0, 0] == 90 and want[5, 0] == 0 and np.isfinite(want[0, 5])


# ------------------------------------------------------------------------------------------------ 7. through the pipeline
@pytest.fixture(scope="module")
def model():
    from cofii2p_amd.network import CoFiI2P
    import bench

    return CoFiI2P(bench.Opt()).to(DEV)


def made_up(i):
    """a camera and a rigid ground-truth pose per frame (float32 values, as a loader hands them over)"""
    K = np.array([[300.0 + 4 * i, 0, 256.0], [0, 296.0 + 2 * i, 80.0 + i], [0, 0, 1.0]], np.float32)
    P = np.eye(4)
    P[:3, :3] = Rotation.from_euler("xzy", [3.0 * i, 5.0 - i, 2.0 + i], degrees=True).as_matrix()
    P[:3, 3] = [0.5 * i, -0.2, 1.0 + 0.1 * i]
    return K, P.astype(np.float32)


def test_eval_into_forward_async(ev, model):
    from cofii2p_amd.network import CoFiI2P
    from cofii2p_amd._lib import CofiError
    import bench

    B, iters, seed = 4, 1000, 11
    frames = bench.make_inputs(torch.device(DEV), list(range(B)), 20480)
    stacked, imgs = CoFiI2P.stack_frames([fr[0] for fr in frames], [fr[1] for fr in frames])
    Kd = torch.from_numpy(np.stack([made_up(f)[0] for f in range(B)])).to(DEV)
    Pd = torch.from_numpy(np.stack([made_up(f)[1] for f in range(B)])).to(DEV)
    ri = torch.arange(B, dtype=torch.int32, device=DEV)
    model.enable_graphs(True)
    try:
        h0 = model.forward_async(61, stacked, imgs, pose_K=Kd, pose_iterations=iters, pose_seed=seed)
        plain = [[t.clone() for t in out] for out in model.finish(h0)]
        pose0 = {k: v.clone() for k, v in h0["pose"].items()}
        table = ev.EvalTable(B, device=DEV)
        h = model.forward_async(61, stacked, imgs, pose_K=Kd, pose_iterations=iters, pose_seed=seed, eval_into=(table, Pd, ri))
        outs = model.finish(h)
        assert set(h) == set(h0)                                         # the handle has the keys it had
        assert set(h["pose"]) == {"result", "R", "t", "inliers"}
        for f in range(B):
            for a, b in zip(outs[f], plain[f]):
                assert torch.equal(a, b), f
        for k in pose0:
            assert torch.equal(h["pose"][k], pose0[k]), k
        rows = table.host()
        t2 = ev.EvalTable(B, device=DEV)
        ev.eval_monitors(h, Kd, Pd, t2)                                  # on the finished handle
        np.testing.assert_array_equal(bits(rows), bits(t2.host()))
        assert not np.isnan(rows[:, :3]).any() and np.all(rows[:, 0] == [o[7].shape[0] for o in outs])
        assert np.array_equal(rows[:, 1], pose0["result"][:, 0].cpu().numpy()) and np.array_equal(rows[:, 2], pose0["result"][:, 1].cpu().numpy())
        with pytest.raises(CofiError):
            model.forward_async(61, stacked, imgs, eval_into=(table, Pd, ri))                       # no pose_K
        with pytest.raises(CofiError):
            model.forward_async(61, stacked, imgs, pose_K=Kd, eval_into=(table, Pd[:3], ri))        # wrong shapes
        with pytest.raises(CofiError):
            model.forward_async(61, stacked, imgs, pose_K=Kd, eval_into=(table, Pd, ri[:2]))
        with pytest.raises(CofiError):
            model.forward_async(61, stacked, imgs, pose_K=Kd, eval_into=(table, Pd.cpu(), ri))      # a CPU tensor
        with pytest.raises(CofiError):
            model.forward_async(61, stacked, imgs, pose_K=Kd, eval_into=(table.rows, Pd, ri))       # not an EvalTable
    finally:
        model.enable_graphs(False)


def test_frame_batcher_and_evaluate(ev, model, tmp_path):
    from cofii2p_amd import metrics, pose as pose_mod
    from cofii2p_amd.serving import FrameBatcher
    import bench

    iters, N = 1000, 6
    frames = bench.make_inputs(torch.device(DEV), list(range(10, 10 + N)), 20480)
    KP = [made_up(i) for i in range(N)]
    thr = metrics.pixel_thresholds()
    model.enable_graphs(True)
    try:
        # FrameBatcher(batch=4) over 6 frames: one full stack, one padded
        table = ev.EvalTable(9, device=DEV)
        fb = FrameBatcher(model, batch=4, streams=2, slot_base=70, pose=True, pose_iterations=iters, eval_table=table)
        tickets = [fb.submit(fr[0], fr[1], K=KP[i][0], P_gt=KP[i][1], row=i) for i, fr in enumerate(frames)]
        fb.drain()
        rows = table.host()
        assert not np.isnan(rows[:N, :3]).any()                          # exactly six rows are written ...
        assert np.all(np.isnan(rows[N:]))                                # ... and the rest of the table stays NaN
        with pytest.raises(ValueError):
            fb.submit(frames[0][0], frames[0][1], K=KP[0][0])            # eval_table needs P_gt and row
        with pytest.raises(ValueError):
            FrameBatcher(model, batch=4, eval_table=table)               # ... and pose=True
        # the same rows per frame from finish() results, with metrics and the single-frame pose errors
        want = np.full((N, 6 + len(thr)), np.nan)
        rels = []
        for i, tk in enumerate(tickets):
            out = fb.result(tk)
            res, R, t, _inl = fb.pose_result(tk)
            fxy = fb.fine_xy(tk).cpu().numpy().astype(np.float64)
            X = out[7].cpu().numpy().astype(np.float64)
            n = X.shape[0]
            ir, rmse = metrics.inlier_ratio_rmse(fxy, X, KP[i][1].astype(np.float64), KP[i][0].astype(np.float64), thr)
            want[i, 0], want[i, 1], want[i, 2] = n, int(res[0]), int(res[1])
            if int(res[0]):
                want[i, 3:5] = pose_mod.pose_errors((R[None], t[None]), KP[i][1][None]).cpu().numpy()[0]
                d = pose_mod.get_P_diff(pose_mod.pose_matrix(R, t), KP[i][1].astype(np.float64))
                assert abs(want[i, 3] - d[0]) <= 1e-9 * max(1.0, d[0]) and abs(want[i, 4] - d[1]) <= 1e-7 * max(1.0, d[1])
            want[i, 5] = rmse
            want[i, 6:] = np.round(ir * n)
            np.testing.assert_array_equal(rows[i, 6:] / n, ir)
            rels.append(abs(rows[i, 5] - rmse) / abs(rmse))
        print("mean residual: relative differences", ["%.2e" % r for r in rels])
        # evaluate() over the six frames, with result files
        samples = [{"pc_data_dict": fr[0], "img": fr[1], "K": torch.from_numpy(KP[i][0]).to(DEV), "P": torch.from_numpy(KP[i][1]).to(DEV)}
                   for i, fr in enumerate(frames)]
        was_training = model.training
        model.train()
        got = ev.evaluate(model, samples, None, batch=4, streams=2, pose_iterations=iters, result_dir=str(tmp_path), slot_base=80)
        assert model.training                                            # eval() for the pass, restored afterwards
        model.train(was_training)
        ref = ev.summarize(want, thr)
        np.testing.assert_array_equal(bits(got["rows"][:, :5]), bits(rows[:N, :5]))
        np.testing.assert_array_equal(bits(got["rows"]), bits(rows[:N]))  # the same frames at the same stack positions: the same rows
        assert np.array_equal(got["n"], ref["n"]) and np.array_equal(got["success"], ref["success"])
        np.testing.assert_array_equal(got["ir"], ref["ir"])
        np.testing.assert_array_equal(bits(got["rte"]), bits(ref["rte"]))
        np.testing.assert_array_equal(bits(got["rre"]), bits(ref["rre"]))
        np.testing.assert_array_equal(bits(got["t_error"]), bits(ref["t_error"]))
        np.testing.assert_array_equal(bits(got["r_error"]), bits(ref["r_error"]))
        assert np.all(np.abs(got["rmse"] - ref["rmse"]) <= 1e-10 * np.abs(ref["rmse"]))
        assert np.abs(got["ir_curve"] - ref["ir_curve"]).max() <= 1e-15 and got["report"] == ref["report"]
        files = sorted(os.listdir(str(tmp_path)))
        assert files == ["%06d.npy" % i for i in range(N)]
        for i, name in enumerate(files):
            d = metrics.load_frame_result(os.path.join(str(tmp_path), name))
            assert tuple(d) == metrics.FRAME_KEYS
            assert tuple(d["fine_xy"].shape) == (2, int(got["n"][i])) and tuple(d["object_points"].shape) == (int(got["n"][i]), 3)
            ir, rmse = metrics.inlier_ratio_rmse(d["fine_xy"], d["object_points"], d["GT_P"], d["K"])   # the file way, in float32
            assert abs(rmse - got["rmse"][i]) <= 1e-3 * max(1.0, abs(rmse))
    finally:
        model.enable_graphs(False)


# ------------------------------------------------------------------------------------------------ 8. arguments
def test_arguments(ev, batch):
    from cofii2p_amd import _lib, ops
    E = _lib.CofiError
    operands = {"object_points": batch["X"], "image_points": batch["uv"], "count": batch["count"], "pose": batch["pose"], "result": batch["result"]}
    t64 = ev.EvalTable(6, thresholds=np.linspace(0, 10, 64), device=DEV)
    ev.eval_monitors(operands, batch["K"], batch["P"], t64)                # T = 64 is served
    assert not np.isnan(t64.host()[:, 6:]).any()
    t65 = ev.EvalTable(6, thresholds=np.linspace(0, 10, 65), device=DEV)
    with pytest.raises(E, match="COFI_EUNSUPPORTED"):
        ev.eval_monitors(operands, batch["K"], batch["P"], t65)
    table = ev.EvalTable(6, device=DEV)
    bad = [dict(operands, object_points=batch["X"].cpu()), dict(operands, object_points=batch["X"].double()),
           dict(operands, image_points=batch["uv"].transpose(1, 2).contiguous()), dict(operands, count=batch["count"].long()),
           dict(operands, count=batch["count"][:5]), dict(operands, pose=batch["pose"][:, :11]), dict(operands, result=batch["result"][:5]),
           {k: v for k, v in operands.items() if k != "pose"}]
    for o in bad:
        with pytest.raises(E):
            ev.eval_monitors(o, batch["K"], batch["P"], table)
    with pytest.raises(E):
        ev.eval_monitors(operands, batch["K"][:5], batch["P"], table)
    with pytest.raises(E):
        ev.eval_monitors(operands, batch["K"], batch["P"][:, :3], table)
    with pytest.raises(E):
        ev.eval_monitors(operands, batch["K"], batch["P"], table, row_index=[0, 1, 2])
    with pytest.raises(E):
        ev.eval_monitors(operands, batch["K"], batch["P"], table.rows)
    with pytest.raises(E):
        ev.EvalTable(4, device="cpu")
    assert np.all(np.isnan(table.host()))                                  # nothing was launched
    # the C entry: NULL operands / bad sizes -> COFI_EINVAL (-1), nothing launched
    lib = _lib.load()
    p = ops._p

    def call(obj=p(batch["X"]), n_max=CAP, frames=6, T=51, table_rows=6, rows=p(table.rows)):
        return lib.cofi_eval_monitors(obj, 3 * CAP, p(batch["uv"]), 2 * CAP, 0, p(batch["count"]), 1, p(batch["K"]), n_max, frames, p(batch["pose"]),
                                      p(batch["result"]), p(batch["P"]), 1, p(table.thresholds), T, p(torch.arange(6, dtype=torch.int32, device=DEV)),
                                      rows, table_rows, ops._stream())

    assert lib.cofi_eval_monitors(None, 0, None, 0, 0, None, 0, None, CAP, 6, None, None, None, 1, None, 51, None, None, 6, ops._stream()) == -1
    assert call(obj=None) == -1 and call(rows=None) == -1 and call(frames=0) == -1 and call(T=0) == -1 and call(table_rows=0) == -1
    assert call(n_max=CAP + 1) == -1                                       # the frame stride is shorter than a frame
    assert call(T=65) == -3
    torch.cuda.synchronize()
    assert np.all(np.isnan(table.host()))
    assert call() == 0
    torch.cuda.synchronize()
    np.testing.assert_array_equal(bits(table.host()), bits(run(ev, batch)))
