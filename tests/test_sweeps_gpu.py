"""Raw nuScenes sweeps on the GPU (cofii2p_amd/sweeps.py; csrc/dataside.hip: cofi_accumulate_sweeps, cofi_voxel_downsample_f64,
cofi_sweeps_to_camera, cofi_resize_image_u8) against tests/sweeps_refs.py, which tests/test_sweeps_refs_cpu.py pins.  Every comparison
is bit for bit, every case runs twice and must give the same bits.  Needs a real MI355X."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import sweeps_refs as R  # noqa: E402
from test_sweeps_refs_cpu import rigid, sample_inputs  # noqa: E402

DEV = "cuda:0"
E = np.float32


@pytest.fixture(scope="module")
def sw():
    from cofii2p_amd import sweeps

    assert torch.cuda.is_available()
    return sweeps


def G(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64, 1: np.uint8}[a.dtype.itemsize])


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(bits(a), bits(b))


def up(v):
    return np.nextafter(E(v), E(np.inf))


def dn(v):
    return np.nextafter(E(v), E(-np.inf))


# ------------------------------------------------------------------------------------------------ accumulation
def run_accumulate(sw, sweeps_in, Ts):
    got = []
    for _ in range(2):
        p, i, n = sw.accumulate(sweeps_in, Ts, device=DEV)
        got.append((p.cpu().numpy(), i.cpu().numpy(), n))
    assert got[0][2] == got[1][2] and same_bits(got[0][0], got[1][0]) and same_bits(got[0][1], got[1][1])
    return got[0]


def check_accumulate(sw, sweeps_in, Ts):
    want_p, want_i = R.accumulate(sweeps_in, Ts)
    p, i, n = run_accumulate(sw, sweeps_in, Ts)
    assert n == want_p.shape[0]
    assert p.dtype == np.float64 and i.dtype == np.float32
    assert same_bits(p, want_p) and same_bits(i, want_i)       # count, order and float64 bits
    return n


def cloud(g, n, ld, reach=4.0):
    rows = g.uniform(-reach, reach, (n, ld)).astype(E)
    rows[:, 3] = g.uniform(0, 255, n).astype(E)
    return rows


def transforms(g, S):
    return np.stack([np.identity(4)] + [rigid(g, 3.0) for _ in range(S - 1)])


def test_accumulate_one_sweep(sw):
    g = np.random.default_rng(10)
    n = check_accumulate(sw, [cloud(g, 700, 5)], transforms(g, 1))
    assert 0 < n < 700


@pytest.mark.parametrize("ld", [4, 5])
def test_accumulate_sweep_and_chunk_boundaries_interleave(sw, ld):
    g = np.random.default_rng(11 + ld)
    sweeps_in = [cloud(g, n, ld) for n in (1023, 1, 0, 1025, 2049)]
    Ts = transforms(g, 5)
    n = check_accumulate(sw, sweeps_in, Ts)
    assert 1000 < n < 4098
    # device tensors take the same path
    want_p, want_i = R.accumulate(sweeps_in, Ts)
    p, i, m = sw.accumulate([G(s) for s in sweeps_in], Ts, device=DEV)
    assert m == n and same_bits(p.cpu().numpy(), want_p) and same_bits(i.cpu().numpy(), want_i)


def test_accumulate_a_sweep_wholly_inside_the_box(sw):
    g = np.random.default_rng(13)
    inside = cloud(g, 1500, 5, reach=0.7)
    assert not R.ego_keep(inside).any()
    far = [cloud(g, n, 5, reach=30.0) for n in (1100, 50)]
    Ts = transforms(g, 3)
    n = check_accumulate(sw, [far[0], inside, far[1]], Ts)
    assert n == int(R.ego_keep(far[0]).sum() + R.ego_keep(far[1]).sum())
    assert check_accumulate(sw, [inside, far[0]], Ts[:2]) == int(R.ego_keep(far[0]).sum())      # ... as the key sweep
    assert check_accumulate(sw, [inside], Ts[:1]) == 0                                            # nothing left at all


def test_accumulate_points_on_the_box_faces(sw):
    rows = []
    for b, other in ((0.8, 1), (2.7, 0)):
        axis = 1 - other
        for v in (E(b), dn(b), up(b), E(-b), up(-b), dn(-b)):
            for o in (E(0.0), E(0.5), E(-0.5)):
                r = np.zeros(5, E)
                r[axis], r[other], r[2], r[3] = v, o, 1.0, len(rows)
                rows.append(r)
    rows = np.stack(rows)
    keep = R.ego_keep(rows)
    assert keep.reshape(2, 6, 3)[:, :, 0].tolist() == [[True, False, True, True, False, True]] * 2
    g = np.random.default_rng(14)
    Ts = transforms(g, 2)
    assert check_accumulate(sw, [rows, rows[::-1].copy()], Ts) == 2 * int(keep.sum())


# ------------------------------------------------------------------------------------------------ voxel grid
def run_voxel(sw, pts, inten, voxel=0.2, cap=None):
    got = []
    for _ in range(2):
        rows, n = sw.voxel_downsample(pts, inten, voxel, cap, device=DEV)
        got.append((rows.cpu().numpy(), n))
    assert got[0][1] == got[1][1] and same_bits(got[0][0], got[1][0])
    return got[0]


def check_voxel(sw, pts, inten, voxel=0.2):
    want, overflow = R.voxel_downsample(pts, inten, voxel)
    assert not overflow
    rows, n = run_voxel(sw, pts, inten, voxel)
    assert n == want.shape[0] and same_bits(rows, want)
    return n


def test_voxel_one_point(sw):
    assert check_voxel(sw, np.array([[1.25, -3.5, 0.125]]), np.array([7.0], E)) == 1


def test_voxel_all_points_in_one_voxel(sw):
    g = np.random.default_rng(20)
    pts = 10.0 + g.uniform(0.0, 0.05, (3000, 3))
    assert check_voxel(sw, pts, g.uniform(0, 255, 3000).astype(E)) == 1


@pytest.mark.parametrize("n", [1500, 5000, 1023, 1024, 1025, 2049])   # the last four: the 1024-row chunk edge
def test_voxel_random_points(sw, n):
    g = np.random.default_rng(21)
    pts = g.uniform(-4.0, 4.0, (n, 3))
    pts[10:200] = pts[3]                                            # a long run
    pts[300:400] = np.round(pts[300:400] * 5) / 5                   # near the lattice
    m = check_voxel(sw, pts, g.uniform(0, 255, n).astype(E))
    assert n // 4 < m < n


def test_voxel_keys_come_from_the_float64_point(sw):
    """boundary_cases: transformed points whose voxel index changes when they are rounded to float32 first, each with a companion at
    the centre of its float64 voxel, and a key-sweep point that fixes the minimum bound.  Accumulated and keyed on the device the
    pairs share a voxel; an implementation that rounds the points to float32 before the key gets more voxels."""
    anchor, T, raw, moved, mate = R.boundary_cases(7)
    k = raw.shape[0]
    assert k >= 8
    key_sweep = np.concatenate([anchor.astype(E), [3.0, 0.0]])[None].astype(E)
    other = np.concatenate([np.concatenate([raw, mate], 0), np.ones((2 * k, 2), E)], 1).astype(E)
    Ts = np.stack([np.identity(4), T])
    pts, inten, n = sw.accumulate([key_sweep, other], Ts, device=DEV)
    assert n == 1 + 2 * k
    host = pts.cpu().numpy()
    assert same_bits(host[1:1 + k], moved)
    want, _ = R.voxel_downsample(host, inten.cpu().numpy(), 0.2)
    rounded, _ = R.voxel_downsample(host.astype(E).astype(np.float64), inten.cpu().numpy(), 0.2)
    assert want.shape[0] <= 1 + k < rounded.shape[0]
    rows, m = run_voxel(sw, pts.clone(), inten.clone())
    assert m == want.shape[0] and same_bits(rows, want)


def test_voxel_cap_smaller_than_the_count(sw):
    g = np.random.default_rng(22)
    pts = g.uniform(-4.0, 4.0, (3000, 3))
    inten = g.uniform(0, 255, 3000).astype(E)
    want, _ = R.voxel_downsample(pts, inten, 0.2)
    rows, n = run_voxel(sw, pts, inten, cap=100)
    assert n == want.shape[0] > 100 and same_bits(rows, want[:100])


def test_voxel_rejects_clouds_wider_than_the_key(sw):
    from cofii2p_amd import _lib

    pts = np.zeros((64, 3))
    pts[1, 0] = 0.2 * 8200
    assert R.voxel_downsample(pts, np.ones(64, E), 0.2)[1]
    with pytest.raises(_lib.CofiError):
        sw.voxel_downsample(pts, np.ones(64, E), device=DEV)
    pts[1, 0] = 0.2 * 8000
    assert check_voxel(sw, pts, np.ones(64, E)) == 2


# ------------------------------------------------------------------------------------------------ camera stage
K_SCALED = R.scaled_K(np.array([[1266.417, 0, 816.267], [0, 1266.417, 491.507], [0, 0, 1]]), 100, 0.4)


def check_camera(sw, rows, P, K, hw):
    want_pc, want_in = R.to_camera(rows, P, K, hw)
    got = []
    for _ in range(2):
        pc, inside = sw.to_camera(rows, P, K, hw, device=DEV)
        got.append((pc.cpu().numpy(), inside))
    assert got[0][1] == got[1][1] and same_bits(got[0][0], got[1][0])
    assert got[0][1] == want_in and same_bits(got[0][0], want_pc)
    return want_in


@pytest.mark.parametrize("M", [1, 257, 5000])
def test_camera_random_rows(sw, M):
    g = np.random.default_rng(30 + M)
    rows = np.concatenate([g.uniform(-20.0, 20.0, (M, 2)), g.uniform(-5.0, 60.0, (M, 1)), g.uniform(0, 255, (M, 1))], 1).astype(E)
    rows[0, 0:3] = [0.5, 0.25, 10.0]
    P = np.identity(4)
    P[0:3, 0:3] = [[np.cos(0.1), 0, np.sin(0.1)], [0, 1, 0], [-np.sin(0.1), 0, np.cos(0.1)]]
    P[0:3, 3] = [0.3, -0.2, 0.1]
    inside = check_camera(sw, rows, P, K_SCALED, (320, 640))
    assert inside >= 1 and (M < 257 or inside < M)


def test_camera_depth_zero_negative_and_picture_borders(sw):
    """P = identity, K = diag(2, 2, 1), z = 1: u = 2 x and v = 2 y exactly, so the borders 0, W - 1, H - 1 and their float32 neighbours
    are hit exactly"""
    H, W = 320, 640
    K = np.diag([2.0, 2.0, 1.0]).astype(E)
    tiny = np.nextafter(E(0), E(-1))
    xs = [(E(0), True), (tiny, False), (E(-1.5), False), (E((W - 1) / 2), True), (up((W - 1) / 2), False), (dn((W - 1) / 2), True)]
    ys = [(E(0), True), (tiny, False), (E((H - 1) / 2), True), (up((H - 1) / 2), False), (dn((H - 1) / 2), True)]
    rows, expect = [], []
    for x, okx in xs:
        rows.append([x, E(10.0), E(1.0), E(1.0)])
        expect.append(okx)
    for y, oky in ys:
        rows.append([E(10.0), y, E(1.0), E(2.0)])
        expect.append(oky)
    for z in (E(0.0), E(-0.0), E(-1.0), dn(0.0)):                  # depth exactly 0 and negative: outside, no division
        rows.append([E(0.0), E(0.0), z, E(3.0)])
        expect.append(False)
    rows = np.asarray(rows, E)
    for n, (r, ok) in enumerate(zip(rows, expect)):
        assert R.to_camera(r[None], np.identity(4), K, (H, W))[1] == int(ok), n
    assert check_camera(sw, rows, np.identity(4), K, (H, W)) == sum(expect)
    for r, ok in zip(rows, expect):                                   # and one by one
        assert sw.to_camera(r[None], np.identity(4), K, (H, W), device=DEV)[1] == int(ok)


# ------------------------------------------------------------------------------------------------ image
@pytest.mark.parametrize("hw,top,out", [((23, 37), 5, (7, 15)), ((900, 1600), 100, (320, 640))])
def test_resize(sw, hw, top, out):
    img = np.random.default_rng(40).integers(0, 256, hw + (3,), dtype=np.uint8)
    want = R.resize_u8(img, top, 0.4)
    a = sw.resize_u8(img, top, 0.4, device=DEV).cpu().numpy()
    b = sw.resize_u8(G(img), top, 0.4, device=DEV).cpu().numpy()
    assert want.shape == out + (3,) and same_bits(a, want) and same_bits(a, b)


# ------------------------------------------------------------------------------------------------ one sample
PPS, MIN_POINTS, MIN_INSIDE = 5000, 25000, 5000     # 7 x 5000 rows: ~30 900 accumulated, ~25 600 voxels, ~5 400 in the front camera


@pytest.fixture(scope="module")
def sample():
    from cofii2p_amd import synth

    s = synth.make_raw_sweeps(1, points_per_sweep=PPS, blind_first=True)
    sweeps_in, Ts, cams = sample_inputs(s)
    want, why = R.build_sample(sweeps_in, Ts, cams[1:], min_points=MIN_POINTS, min_inside=MIN_INSIDE)
    assert why is None
    return sweeps_in, Ts, cams, want


def assert_sample(got, want):
    assert set(got) == set(want)
    for k in ("inside", "accumulated", "voxels", "camera"):
        assert got[k] == want[k] and isinstance(got[k], int), k
    assert same_bits(got["pc"].cpu().numpy(), want["pc"]) and same_bits(got["img"].cpu().numpy(), want["img"])
    assert same_bits(got["K"], want["K"]) and same_bits(got["P"], want["P"])


def test_build_sample_equals_the_restatement(sw, sample):
    sweeps_in, Ts, cams, want = sample
    for _ in range(2):
        got = sw.build_sample(sweeps_in, Ts, cams[1:], None, MIN_POINTS, MIN_INSIDE, device=DEV)
        assert_sample(got, want)
    assert want["accumulated"] > want["voxels"] >= MIN_POINTS and want["inside"] > MIN_INSIDE and want["camera"] == 0
    assert sw.build_sample.last["inside"] == [want["inside"]] and "rejected" not in sw.build_sample.last


def test_build_sample_takes_the_second_candidate(sw, sample):
    sweeps_in, Ts, cams, want = sample
    got = sw.build_sample(sweeps_in, Ts, cams, None, MIN_POINTS, MIN_INSIDE, device=DEV)
    assert_sample(got, dict(want, camera=1))
    assert len(sw.build_sample.last["inside"]) == 2 and sw.build_sample.last["inside"][0] <= MIN_INSIDE
    ref, _ = R.build_sample(sweeps_in, Ts, cams, min_points=MIN_POINTS, min_inside=MIN_INSIDE)
    assert ref["camera"] == 1


@pytest.mark.parametrize("min_points,min_inside,why", [(10 ** 6, MIN_INSIDE, "accumulated"), (28000, MIN_INSIDE, "voxels"), (MIN_POINTS, 6000, "inside")])
def test_build_sample_rejections(sw, sample, min_points, min_inside, why):
    sweeps_in, Ts, cams, want = sample
    assert R.build_sample(sweeps_in, Ts, cams, min_points=min_points, min_inside=min_inside) == (None, why)
    assert sw.build_sample(sweeps_in, Ts, cams, None, min_points, min_inside, device=DEV) is None
    last = sw.build_sample.last
    assert last["rejected"] == why and last["accumulated"] == want["accumulated"]
    assert ("voxels" in last) == (why != "accumulated") and ("inside" in last) == (why == "inside")


def test_build_sample_feeds_the_preparer(sw, sample):
    """the device sample through FramePreparer(dataset='nuscenes') == the restatement's host arrays through it"""
    from cofii2p_amd import dataside
    from test_dataside_cpu import nuscenes_opt
    from test_dataside_normals_gpu import assert_same

    sweeps_in, Ts, cams, want = sample
    s = sw.build_sample(sweeps_in, Ts, cams[1:], None, MIN_POINTS, MIN_INSIDE, device=DEV)
    opt = nuscenes_opt()
    a = dataside.FramePreparer(opt, DEV, dataset="nuscenes").prepare(s["pc"], s["img"], s["K"], None, 5)
    b = dataside.FramePreparer(opt, DEV, dataset="nuscenes").prepare(want["pc"], want["img"], want["K"], None, 5)
    assert tuple(a["img"].shape) == (3, 160, 320) and a["pc_data_dict"]["points"][0].shape[0] == opt.num_pc
    assert_same(a, b)


# ------------------------------------------------------------------------------------------------ argument errors
def test_argument_errors(sw):
    """every entry refuses NULL and misaligned operands and a missing, misaligned or short workspace before it launches anything"""
    from cofii2p_amd import _lib

    lib = _lib.load()
    EINVAL, EWS = _lib.COFI_EINVAL, _lib.COFI_EWORKSPACE
    n = 2048
    rows = torch.zeros((n, 5), dtype=torch.float32, device=DEV)
    offs = torch.tensor([0, n], dtype=torch.int32, device=DEV)
    T = torch.zeros((2, 4, 4), dtype=torch.float64, device=DEV)
    pts = torch.zeros((n, 3), dtype=torch.float64, device=DEV)
    inten = torch.zeros((n,), dtype=torch.float32, device=DEV)
    cnt = torch.zeros(4, dtype=torch.int32, device=DEV)
    out4 = torch.zeros((n + 1, 4), dtype=torch.float32, device=DEV)
    ws = torch.zeros(1 << 22, dtype=torch.uint8, device=DEV)
    p = lambda t: t.data_ptr()

    need = lib.cofi_accumulate_sweeps_workspace(n)
    assert 0 < need <= ws.numel() and lib.cofi_accumulate_sweeps_workspace(0) == 0
    acc = lambda **kw: lib.cofi_accumulate_sweeps(*[kw.get(k, d) for k, d in (("rows", p(rows)), ("ld", 5), ("offs", p(offs)), ("S", 1), ("total", n), ("T", p(T)),
                                                                         ("pts", p(pts)), ("inten", p(inten)), ("cnt", p(cnt)), ("ws", p(ws)),
                                                                         ("bytes", ws.numel()), ("stream", None))])
    for kw in ({"rows": None}, {"offs": None}, {"T": None}, {"pts": None}, {"inten": None}, {"cnt": None}, {"ld": 3}, {"ld": 6}, {"S": 0}, {"S": 65},
               {"total": 0}, {"T": p(T) + 4}, {"pts": p(pts) + 4}):
        assert acc(**kw) == EINVAL, kw
    for kw in ({"ws": None}, {"ws": p(ws) + 4}, {"bytes": need - 1}):
        assert acc(**kw) == EWS, kw

    need = lib.cofi_voxel_downsample_f64_workspace(n)
    assert 0 < need <= ws.numel() and lib.cofi_voxel_downsample_f64_workspace(0) == 0
    vox = lambda **kw: lib.cofi_voxel_downsample_f64(*[kw.get(k, d) for k, d in (("pts", p(pts)), ("inten", p(inten)), ("N", n), ("voxel", 0.2), ("out", p(out4)),
                                                                            ("cap", n), ("cnt", p(cnt)), ("ws", p(ws)), ("bytes", ws.numel()), ("stream", None))])
    for kw in ({"pts": None}, {"inten": None}, {"out": None}, {"cnt": None}, {"N": 0}, {"voxel": 0.0}, {"voxel": float("nan")}, {"cap": 0},
               {"pts": p(pts) + 4}, {"out": p(out4) + 4}):
        assert vox(**kw) == EINVAL, kw
    for kw in ({"ws": None}, {"ws": p(ws) + 8}, {"bytes": need - 1}):
        assert vox(**kw) == EWS, kw

    P = torch.eye(4, dtype=torch.float64, device=DEV)
    K = torch.eye(3, dtype=torch.float32, device=DEV)
    cloud4 = torch.zeros((4, n), dtype=torch.float32, device=DEV)
    cam = lambda **kw: lib.cofi_sweeps_to_camera(*[kw.get(k, d) for k, d in (("rows", p(out4)), ("M", n), ("P", p(P)), ("K", p(K)), ("H", 320), ("W", 640),
                                                                        ("out", p(cloud4)), ("cnt", p(cnt)), ("stream", None))])
    for kw in ({"rows": None}, {"P": None}, {"K": None}, {"out": None}, {"cnt": None}, {"M": 0}, {"H": 0}, {"W": 0}, {"rows": p(out4) + 4}, {"P": p(P) + 4}):
        assert cam(**kw) == EINVAL, kw

    img = torch.zeros((20, 30, 3), dtype=torch.uint8, device=DEV)
    dst = torch.zeros((8, 12, 3), dtype=torch.uint8, device=DEV)
    rs = lambda **kw: lib.cofi_resize_image_u8(*[kw.get(k, d) for k, d in (("src", p(img)), ("sh", 20), ("sw", 30), ("top", 0), ("dh", 8), ("dw", 12),
                                                                      ("dst", p(dst)), ("stream", None))])
    for kw in ({"src": None}, {"dst": None}, {"sh": 0}, {"sw": 0}, {"top": -1}, {"top": 20}, {"dh": 0}, {"dw": 0}):
        assert rs(**kw) == EINVAL, kw
    torch.cuda.synchronize()
    assert not cnt.any().item()                                     # nothing was launched

    # ... and the wrappers refuse what the entries cannot take
    with pytest.raises(_lib.CofiError):
        sw.accumulate([np.zeros((4, 3), E)], np.identity(4)[None], device=DEV)
    with pytest.raises(_lib.CofiError):
        sw.accumulate([np.zeros((4, 5), E)] * 65, np.zeros((65, 4, 4)), device=DEV)
    with pytest.raises(_lib.CofiError):
        sw.to_camera(np.zeros((4, 3), E), np.identity(4), np.identity(3), (8, 8), device=DEV)
    with pytest.raises(_lib.CofiError):
        sw.resize_u8(np.zeros((4, 4, 3), np.uint8), 4, 0.5, device=DEV)
