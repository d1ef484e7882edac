"""Scans without normals through the data side (cofii2p_amd/dataside.py, normals='estimate'): a (4, N) KITTI scan [xyz | intensity] is
prepared exactly as the (7, N) scan that carries the normals cofii2p_amd.normals.estimate_normals computes for the same points; the
default normals='given' and the nuScenes path are unchanged.  Needs a real MI355X.

"Bit-equal in every returned tensor" leaves out one entry by necessity: pc_data_dict['order'], the k-nearest grid's cell order of each stage.
It is a processing-order hint whose order inside a cell is whatever the scatter's atomics made it (csrc/knn_grid.hip: "order inside a
cell is arbitrary: the result does not depend on it"), so two preparations of the SAME frame differ in it; it is compared as a permutation."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import dataside_oracle as D  # noqa: E402
from test_dataside_cpu import kitti_opt, nuscenes_opt  # noqa: E402

DEV = "cuda:0"
INDEX = 4


def G(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def calib_P_Tr():
    from cofii2p_amd import dataside, synth

    cal = dataside.calib_matrices(synth.KITTI_CALIB_LINES)
    return np.dot(cal["P2"], cal["Tr"])


def assert_same(a, b, path="sample"):
    """every tensor of two sample dicts bit-equal, everything else equal"""
    if isinstance(a, dict):
        assert set(a) == set(b), path
        for key in a:
            if key == "order":      # cell order of the k-nearest grid: arbitrary inside a cell, see the module docstring
                assert len(a[key]) == len(b[key]), path
                for x, y in zip(a[key], b[key]):
                    assert x.dtype == y.dtype and torch.equal(torch.sort(x).values, torch.sort(y).values), path + "['order']"
                continue
            assert_same(a[key], b[key], "%s[%r]" % (path, key))
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), path
        for i, (x, y) in enumerate(zip(a, b)):
            assert_same(x, y, "%s[%d]" % (path, i))
    elif torch.is_tensor(a):
        assert a.dtype == b.dtype and torch.equal(a, b), path
    elif isinstance(a, np.ndarray):
        assert np.array_equal(a, b), path
    else:
        assert a == b, path


@pytest.fixture(scope="module")
def frame():
    """one 6000-point scan, its estimated normals, and the two prepared samples compared below (computed once)"""
    from cofii2p_amd import dataside, normals, synth

    data, img, K = synth.make_raw_scan(3, num_points=6000)
    P_Tr = calib_P_Tr()
    n = normals.estimate_normals(G(data[:3].T))
    with_normals = data.copy()
    with_normals[4:7] = n.cpu().numpy().T
    prep = dataside.FramePreparer(kitti_opt(), DEV, normals="estimate")
    estimated = prep.prepare(np.ascontiguousarray(data[:4]), img, K, P_Tr, INDEX)
    given = dataside.FramePreparer(kitti_opt(), DEV).prepare(with_normals, img, K, P_Tr, INDEX)
    return {"data": data, "img": img, "K": K, "P_Tr": P_Tr, "with_normals": with_normals, "estimated": estimated, "given": given, "last": dict(prep.last)}


def test_scan_without_normals_equals_scan_with_estimated_normals(frame):
    assert_same(frame["estimated"], frame["given"])
    feats = frame["estimated"]["pc_data_dict"]["feats"]
    assert tuple(feats.shape) == (20480, 4) and torch.isfinite(feats).all()
    assert not np.array_equal(frame["with_normals"][4:7], frame["data"][4:7])      # the scan's stored normals played no part


def test_stored_normals_are_ignored_when_estimating(frame):
    from cofii2p_amd import dataside

    prep = dataside.FramePreparer(kitti_opt(), DEV, normals="estimate")
    junk = frame["data"].copy()
    junk[4:7] = 9.0
    assert_same(prep.prepare(G(junk), frame["img"], frame["K"], frame["P_Tr"], INDEX), frame["estimated"])
    assert (junk[4:7] == 9.0).all()
    # the voxel table through the public half as well: (4, N) in, the table of the (7, N) scan out
    vox_e, n_e = prep.voxel_downsample(G(frame["data"][:4]), G(frame["P_Tr"].astype(np.float32)))
    vox_g, n_g = dataside.FramePreparer(kitti_opt(), DEV).voxel_downsample(G(frame["with_normals"]), G(frame["P_Tr"].astype(np.float32)))
    assert n_e == n_g == frame["last"]["voxels"] and torch.equal(vox_e[:n_e], vox_g[:n_g])


def test_features_of_single_point_voxels_are_unit_normals(frame):
    """a voxel that holds one point hands its normal on unchanged (rotated twice); a voxel of several points averages them"""
    data, P_Tr = frame["data"], frame["P_Tr"]
    pts = D.rigid(P_Tr, data[0:3]).T.astype(np.float64)                # the voxel index of oracle/dataside_oracle.py::voxel_down_sample
    vidx = np.floor((pts - (pts.min(0) - 0.05)) / 0.1).astype(np.int64)
    key = (vidx[:, 0] << 26) | (vidx[:, 1] << 13) | vidx[:, 2]
    _, counts = np.unique(key, return_counts=True)                     # ascending keys: the order of the voxel table
    assert len(counts) == frame["last"]["voxels"]
    single = counts[frame["last"]["choice"]] == 1
    norm = np.linalg.norm(frame["estimated"]["pc_data_dict"]["feats"][:, 1:4].cpu().numpy().astype(np.float64), axis=1)
    assert single.sum() > 1000 and (~single).sum() > 50
    assert np.abs(norm[single] - 1.0).max() <= 1e-5
    assert norm.max() <= 1.0 + 1e-5


def test_given_still_needs_the_normals(frame):
    from cofii2p_amd import _lib, dataside

    prep = dataside.FramePreparer(kitti_opt(), DEV)
    with pytest.raises(_lib.CofiError, match=r"contiguous \(7, N\) float32"):
        prep.prepare(np.ascontiguousarray(frame["data"][:4]), frame["img"], frame["K"], frame["P_Tr"], INDEX)
    with pytest.raises(_lib.CofiError):
        dataside.FramePreparer(kitti_opt(), DEV, normals="estimate").voxel_downsample(G(frame["data"][:5]), G(frame["P_Tr"].astype(np.float32)))
    with pytest.raises(ValueError):
        dataside.FramePreparer(kitti_opt(), DEV, normals="computed")


def test_nuscenes_path_is_untouched():
    from cofii2p_amd import dataside, synth

    pc4, img, K = synth.make_raw_nuscenes(1, 6000)
    opt = nuscenes_opt()
    plain = dataside.FramePreparer(opt, DEV, dataset="nuscenes").prepare(pc4, img, K, None, 2)
    for kw in (dict(normals="given"), dict(normals="estimate", normals_k=16, normals_radius=0.5)):
        assert_same(dataside.FramePreparer(opt, DEV, dataset="nuscenes", **kw).prepare(pc4, img, K, None, 2), plain)


def test_loader_frame_with_estimated_normals(frame):
    from cofii2p_amd.loader import FrameLoader
    from test_dataside_cpu import INT_KEYS

    loader = FrameLoader(kitti_opt(), DEV, slots=1, workers=1, capture_stream=torch.cuda.Stream(device=DEV), normals="estimate")
    try:
        assert loader.preps[0].normals == "estimate" and loader.preps[0].normals_k == 30 and loader.preps[0].normals_radius is None
        loader.begin(0, np.ascontiguousarray(frame["data"][:4]), frame["img"], frame["K"], frame["P_Tr"], INDEX)
        smp = loader.complete(0)
        smp["finish_labels"]()
        torch.cuda.synchronize()
        want, dd = frame["estimated"], smp["pc_data_dict"]
        assert torch.equal(smp["img"], want["img"]) and torch.equal(dd["feats"], want["pc_data_dict"]["feats"])
        for i in range(5):
            assert torch.equal(dd["points"][i], want["pc_data_dict"]["points"][i])
            assert torch.equal(dd["neighbors"][i].long(), want["pc_data_dict"]["neighbors"][i])
        for key in INT_KEYS + ("coarse_img_mask", "K", "K_4", "P"):
            assert torch.equal(smp[key], want[key]), key
        loader.release(0)
    finally:
        loader.close()
