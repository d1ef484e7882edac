"""The float64 reference of the pose covariance (tests/pose_cov_refs.py) held to calculus, to oracle/pnp_oracle.py and tests/rig_pose_refs.py,
to the statistics it claims (a calibrated NEES), and the host-only parts of the surface (transport_covariance, covariance_sigmas, header
and binding table)."""
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import pnp_oracle as po
import pose_cov_refs as pc
import rig_pose_refs as rr
from cofii2p_amd import _lib, pose


def p12(R, t):
    return np.concatenate([np.asarray(R, np.float64).reshape(9), np.asarray(t, np.float64)])


# ------------------------------------------------------------------------------------------------ the Jacobian
@pytest.mark.parametrize("form", ["frame", "rig"])
def test_jacobian_is_the_derivative_of_the_residual(form):
    """J of row_terms against central differences of the residual under se3_update, every row and every direction; the rig form through
    extrinsics that are far from the identity"""
    sc = rr.rig_scene(9, (6, 7, 5), noise=2.0, outliers=0.0)
    R, t = sc["T"]
    c = 1
    E = sc["E"][c] if form == "rig" else None
    assert form == "frame" or np.abs(sc["E"][c][:, :3] - np.eye(3)).max() > 0.5
    if form == "frame":      # the camera's own pose
        R, t = rr.compose(sc["E"][c], (R, t))
    X, uv, K4 = sc["Xs"][c], sc["uvs"][c], sc["K4s"][c]
    r0, J, z = pc.row_terms(R, t, X, uv, K4, E)
    assert (z > 1.0).all()
    h = 1e-6
    for k in range(6):
        d = np.zeros(6)
        d[k] = h
        rp = pc.row_terms(*po.se3_update(R, t, d), X, uv, K4, E)[0]
        rm = pc.row_terms(*po.se3_update(R, t, -d), X, uv, K4, E)[0]
        fd = (rp - rm) / (2 * h)
        assert np.abs(fd - J[:, :, k]).max() <= 1e-6 * max(1.0, np.abs(J[:, :, k]).max()), (form, k, np.abs(fd - J[:, :, k]).max())


def test_normal_equations_are_the_refits():
    """H and cost of the restatement are those oracle/pnp_oracle.py::refine and rig_pose_refs.rig_cost_and_normal minimise"""
    sc = rr.rig_scene(10, (12, 9, 8), noise=1.0, outliers=0.0)
    R, t = sc["T"]
    ne = pc.normal_equations(p12(R, t), pc.rig_cams(sc["Xs"], sc["uvs"], sc["K4s"], sc["E"]))
    cost, H, _ = rr.rig_cost_and_normal(R, t, sc["Xs"], sc["uvs"], sc["K4s"], sc["E"])
    assert ne["n"] == 29 and abs(ne["cost"] - cost) <= 1e-10 * cost and np.abs(ne["H"] - H).max() <= 1e-10 * np.abs(H).max()
    assert (np.abs(ne["H"]) <= ne["absH"] * (1 + 1e-12)).all()


# ------------------------------------------------------------------------------------------------ rig at C = 1
def test_one_camera_with_identity_extrinsics_is_the_frame_form():
    X, uv, truth = pc.calibration_scene()[0]
    pose12 = pc.pose12_f32(*truth)
    mask = np.arange(len(X)) % 3 != 0
    a = pc.covariance(pose12, [1], [pc.frame_cam(X, uv, pc.CAL_K4, mask)])
    b = pc.covariance(pose12, [1], pc.rig_cams([X], [uv], [pc.CAL_K4], rr.IDENTITY_E[None], [mask]))
    assert a["stat"][0] == 1 and a["n"] == int(mask.sum())
    for k in ("cov", "info", "stat"):
        assert np.array_equal(a[k], b[k]), k          # the identity multiplies by 1 and adds 0: exact
    assert np.array_equal(a["cov"], a["cov"].T) and np.array_equal(a["info"], a["info"].T)
    assert np.abs(a["cov"] @ a["info"] - np.eye(6)).max() <= 1e-9 * a["kappa"]


# ------------------------------------------------------------------------------------------------ transport
def test_transport_is_the_covariance_in_the_cameras_own_tangent_space():
    sc = rr.rig_scene(14, (30, 25, 20), noise=1.0, outliers=0.0)
    T = sc["T"]
    for c in range(3):
        E = sc["E"][c]
        X, uv, K4 = sc["Xs"][c], sc["uvs"][c], sc["K4s"][c]
        rig = pc.covariance(p12(*T), [1], pc.rig_cams([X], [uv], [K4], [E]), sigma_px=1.0)
        cam = pc.covariance(p12(*rr.compose(E, T)), [1], [pc.frame_cam(X, uv, K4)], sigma_px=1.0)
        assert rig["stat"][0] == 1 and cam["stat"][0] == 1 and cam["kappa"] < 1e6
        want, moved = cam["cov"], pc.transport(rig["cov"], E)
        dg = np.sqrt(np.diag(want))
        assert np.abs(moved - want).max() > 0 and (np.abs(moved - want) <= 1e-9 * cam["kappa"] * dg[:, None] * dg[None, :]).all(), c
        assert np.abs(rig["cov"] - want).max() > 1e-3 * np.abs(want).max()          # the transport is no identity here
        got = pose.transport_covariance(torch.from_numpy(rig["cov"]), E)
        assert got.dtype == torch.float64 and torch.equal(got, got.T)
        assert (np.abs(got.numpy() - moved) <= 1e-12 * dg[:, None] * dg[None, :]).all()
        E4 = np.vstack([E, [0, 0, 0, 1.0]])
        both = pose.transport_covariance(torch.from_numpy(np.stack([rig["cov"], 2 * rig["cov"]])), torch.from_numpy(E4))
        assert tuple(both.shape) == (2, 6, 6)                                      # a stack of covariances, E as (4,4)
        for k in range(2):
            assert (np.abs(both[k].numpy() - (k + 1) * moved) <= (k + 1) * 1e-12 * dg[:, None] * dg[None, :]).all(), k
        rot, tra = pose.covariance_sigmas(got)
        assert abs(float(rot) - pc.sigmas(moved)[0]) <= 1e-12 * float(rot) and abs(float(tra) - pc.sigmas(moved)[1]) <= 1e-12 * float(tra)
    with pytest.raises(_lib.CofiError):
        pose.transport_covariance(torch.zeros(5, 5), sc["E"][0])
    with pytest.raises(_lib.CofiError):
        pose.transport_covariance(torch.zeros(6, 6), np.eye(3))


# ------------------------------------------------------------------------------------------------ calibration
@pytest.mark.parametrize("sigma_px", [None, 1.0], ids=["estimated", "given"])
def test_nees_is_calibrated(sigma_px):
    """64 trials, 200 matches, 1 px noise, refit from the truth, pose rounded to float32: the mean NEES is that of a chi-square with 6
    degrees of freedom (expected 6, standard error sqrt(12 / 64) = 0.43)"""
    vals, kappas = [], []
    for X, uv, truth in pc.calibration_scene():
        R, t = po.refine(truth[0], truth[1], X, uv, pc.CAL_K4)
        pose12 = pc.pose12_f32(R, t)
        ref = pc.covariance(pose12, [1], [pc.frame_cam(X, uv, pc.CAL_K4)], sigma_px)
        assert ref["stat"][0] == 1 and ref["stat"][1] == pc.CAL_N and 0 < ref["stat"][3] <= 1
        assert 0.7 < ref["stat"][2] < 1.4, ref["stat"][2]                          # the pixel variance that was put in
        vals.append(pc.nees(pose12, rr.pose_matrix(*truth), ref["info"], ref["stat"]))
        kappas.append(ref["kappa"])
    mean = float(np.mean(vals))
    print("NEES %s: mean %.3f, min %.2f, max %.2f; kappa %.0f - %.0f" % (sigma_px, mean, min(vals), max(vals), min(kappas), max(kappas)))
    assert 4.5 <= mean <= 7.5, mean
    assert max(kappas) <= 1e6


def test_tangent_error_inverts_the_update():
    rng = np.random.default_rng(3)
    for _ in range(8):
        R, t = pc.rotvec_matrix(rng.normal(size=3) * 0.5), rng.normal(size=3)
        d = np.concatenate([rng.normal(size=3) * 0.2, rng.normal(size=3)])
        Rg, tg = po.se3_update(R, t, d)
        assert np.abs(pc.tangent_error(p12(R, t), rr.pose_matrix(Rg, tg)) - d).max() <= 1e-13
    assert np.isnan(pc.nees(p12(R, t), np.eye(4), np.eye(6), np.zeros(4)))


# ------------------------------------------------------------------------------------------------ failure cases
def assert_failed(ref, n=None):
    assert ref["stat"][0] == 0 and ref["stat"][3] == 0 and np.isfinite(ref["stat"]).all()
    assert not ref["cov"].any() and not ref["info"].any()
    if n is not None:
        assert ref["stat"][1] == n


def test_failure_cases():
    X, uv, truth = pc.calibration_scene()[1]
    pose12 = pc.pose12_f32(*truth)
    cam = pc.frame_cam(X, uv, pc.CAL_K4)
    assert pc.covariance(pose12, [1, 200, 0], [cam])["stat"][0] == 1
    assert_failed(pc.covariance(pose12, [0, 0, -1], [cam]), 0)                              # the solver failed
    three = dict(cam, mask=np.arange(len(X)) < 3)
    assert_failed(pc.covariance(pose12, [1], [three]), 3)                                    # 2 n - 6 = 0 with sigma estimated
    given = pc.covariance(pose12, [1], [three], sigma_px=1.0)
    assert given["stat"][0] == 1 and given["stat"][1] == 3 and given["stat"][2] == 0 and np.isfinite(given["cov"]).all()
    four = pc.frame_cam(np.repeat(X[:1], 4, 0), np.repeat(uv[:1], 4, 0), pc.CAL_K4)
    assert_failed(pc.covariance(pose12, [1], [four]), 4)                                     # four copies of one point: rank 2
    assert_failed(pc.covariance(pose12, [1], [four], sigma_px=1.0), 4)
    none = dict(cam, mask=np.zeros(len(X), bool))
    assert_failed(pc.covariance(pose12, [1], [none]), 0)                                     # a mask that selects nothing
    assert_failed(pc.covariance(pose12, [1], [none], sigma_px=1.0), 0)
    assert_failed(pc.covariance(pose12, [1], [dict(cam, K4=(0.0, 400.0, 128.0, 40.0))]), 0)   # unusable intrinsics
    behind = X.copy()
    behind[7] = -behind[7]                                                                   # one row behind the camera: skipped, not counted
    ref = pc.covariance(pose12, [1], [pc.frame_cam(behind, uv, pc.CAL_K4)])
    assert ref["stat"][0] == 1 and ref["stat"][1] == len(X) - 1


# ------------------------------------------------------------------------------------------------ host-only checks
NEW = ("cofi_pose_covariance", "cofi_pose_covariance_batch", "cofi_pose_covariance_rig", "cofi_pose_nees")


def test_header_and_binding_table():
    assert set(_lib.header_symbols()) == set(_lib.SIGNATURES)
    assert set(NEW) <= set(_lib.SIGNATURES)
    assert _lib.ABI_VERSION == 3                                                 # an additive change
    header = (Path(__file__).resolve().parents[1] / "include" / "cofi_hip.h").read_text()
    assert re.search(r"#define COFI_ABI_VERSION 3\b", header)
    for name in NEW + ("cofi_pnp_ransac", "cofi_pnp_ransac_batch", "cofi_pnp_ransac_rig"):
        m = re.search(r"\b%s\(([^;]*)\);" % name, header)
        assert m, name
        assert len(m.group(1).split(",")) == len(_lib.SIGNATURES[name][1]), name
    sig = _lib.SIGNATURES
    # the solver's operands up to the iteration count, then pose, result, mask, sigma_px, cov, info, stat, stream
    assert sig["cofi_pose_covariance"][1][:8] == sig["cofi_pnp_ransac"][1][:8] and len(sig["cofi_pose_covariance"][1]) == 8 + 8
    assert sig["cofi_pose_covariance_batch"][1][:10] == sig["cofi_pnp_ransac_batch"][1][:10] and len(sig["cofi_pose_covariance_batch"][1]) == 10 + 8
    assert sig["cofi_pose_covariance_rig"][1][:13] == sig["cofi_pnp_ransac_rig"][1][:13] and len(sig["cofi_pose_covariance_rig"][1]) == 13 + 8
    assert not any(name.endswith("_workspace") for name in sig if name.startswith("cofi_pose_"))      # none of them needs one


def test_python_surface_refuses_before_loading_anything():
    for name in ("pose_covariance", "pose_covariance_batch", "pose_covariance_batch_into", "pose_covariance_rig", "pose_covariance_rig_into",
                 "pose_nees", "transport_covariance", "covariance_sigmas"):
        assert callable(getattr(pose, name)), name
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(_lib.CofiError):
            pose._sigma(bad)
    assert pose._sigma(None) == 0.0 and pose._sigma(True) == 0.0 and pose._sigma(2) == 2.0
    from cofii2p_amd.serving import FrameBatcher

    with pytest.raises(ValueError):
        FrameBatcher(None, covariance=True)                                      # needs pose=True, as fuse does
    with pytest.raises(ValueError):
        FrameBatcher(None, pose=True, sigma_px=1.0)                              # sigma_px goes with covariance
    with pytest.raises(ValueError):
        FrameBatcher(None, pose=True, covariance=True, sigma_px=0.0)
    rot, tra = pose.covariance_sigmas(torch.diag(torch.tensor([1e-6, 4e-6, 4e-6, 0.01, 0.02, 0.06], dtype=torch.float64)))
    assert abs(float(rot) - np.degrees(3e-3)) < 1e-12 and abs(float(tra) - 0.3) < 1e-15
