"""Sub-pixel fine matches without a GPU: the binding table, the float64 restatement of cofi_fine_refine (tests/fine_refine_refs.py)
against the truth of planted scenes, the seeds of the GPU pose test, and the refusals of the Python surface."""
import functools
import inspect
import re
from pathlib import Path

import numpy as np
import pytest

import fine_refine_refs as fr
from cofii2p_amd import _lib


def test_header_and_binding_table():
    assert set(_lib.header_symbols()) == set(_lib.SIGNATURES)
    assert "cofi_fine_refine" in _lib.SIGNATURES
    assert _lib.ABI_VERSION == 3                                                 # an additive change
    header = (Path(__file__).resolve().parents[1] / "include" / "cofi_hip.h").read_text()
    assert re.search(r"#define COFI_ABI_VERSION 3\b", header)
    m = re.search(r"\bcofi_fine_refine\(([^;]*)\);", header)
    assert m
    params = [p.strip() for p in m.group(1).split(",")]
    sig = _lib.SIGNATURES["cofi_fine_refine"][1]
    assert len(params) == len(sig) == 17
    for p, c in zip(params, sig):   # pointers, ints and the one float sit where the header has them
        want = _lib._P if ("*" in p or p.startswith("cofi_stream_t")) else (_lib._F if p.startswith("float") else _lib._I)
        assert c is want, p
    assert "not written" in header[m.start() - 2500:m.start()].lower()           # rows at or beyond the count: said in the header


@functools.lru_cache(maxsize=None)
def scene(seed, ell):
    sc = fr.planted_scene(seed, ell)
    hard, sub = fr.scene_matches(sc)
    return sc, hard, sub


def test_zero_offsets_give_the_geometric_decode():
    sc, _, _ = scene(0, 1.0)
    n = len(sc["X"])
    rng = np.random.default_rng(5)
    best = rng.integers(0, 16, n).astype(np.int32)
    ref = fr.fine_refine_ref(sc["fmap"], sc["H2"], sc["W2"], sc["coarse_xy"], sc["desc"], best, n, 4.0, zero_delta=True)
    left = np.floor(sc["coarse_xy"][0] * 4.0 - 2.0)
    top = np.floor(sc["coarse_xy"][1] * 4.0 - 2.0)
    assert np.array_equal(ref["sub_xy"][0], left + best % 4) and np.array_equal(ref["sub_xy"][1], top + best // 4)
    # ... which is NOT fine_xy's decode (x + best // 4, y + best % 4) wherever best // 4 != best % 4
    off = best // 4 != best % 4
    assert off.any() and np.all((ref["sub_xy"][0] != left + best // 4)[off])
    # and with the offsets on, a point never leaves its cell
    full = fr.fine_refine_ref(sc["fmap"], sc["H2"], sc["W2"], sc["coarse_xy"], sc["desc"], best, n, 4.0)
    assert np.all(np.abs(full["sub_xy"] - ref["sub_xy"]) <= 0.5)
    # rows at or beyond the count stay unwritten
    part = fr.fine_refine_ref(sc["fmap"], sc["H2"], sc["W2"], sc["coarse_xy"], sc["desc"], best, 10, 4.0)
    assert np.isnan(part["sub_xy"][:, 10:]).all() and np.isnan(part["peak"][10:]).all() and np.isfinite(part["sub_xy"][:, :10]).all()


def test_parabola_rule():
    assert fr.parabola_offset(0.5, 1.0, 0.5) == (0.0, -1.0)
    d, den = fr.parabola_offset(0.2, 1.0, 0.6)          # the peak leans towards the larger neighbour
    assert den < 0 and 0 < d < 0.5 and abs(d - 0.5 * (0.2 - 0.6) / den) < 1e-15
    assert fr.parabola_offset(0.3, 0.3, 0.3) == (0.0, 0.0)                       # flat: den == 0 exactly
    assert fr.parabola_offset(0.1, 0.2, 0.3)[0] == 0.5                           # strictly rising: den == 0 or rounding, half a cell up
    assert fr.parabola_offset(0.9, 0.2, 0.1)[0] == -0.5                          # a larger neighbour, den > 0
    d, den = fr.parabola_offset(1.0, 0.8, 0.5)         # concave, but the vertex lies 2.5 cells away: clamped
    assert den < 0 and d == -0.5
    for bad in ((np.nan, 1.0, 0.5), (0.5, np.nan, 0.5), (0.5, 1.0, np.nan)):
        assert fr.parabola_offset(*bad)[0] == 0.0


@pytest.mark.parametrize("ell", [0.7, 1.0, 1.5])
def test_refined_points_halve_the_quantisation_error(ell):
    eh, er = [], []
    for seed in range(4):
        sc, hard, sub = scene(seed, ell)
        eh.append(hard - sc["uv"])
        er.append(sub - sc["uv"])
    rh, rr = (float(np.sqrt(np.mean(np.concatenate(e) ** 2))) for e in (eh, er))
    print("ell %.1f: hard arg-max %.3f cells rms per axis, refined %.3f, ratio %.2f" % (ell, rh, rr, rr / rh))
    assert 0.25 < rh < 0.33          # the uniform quantisation error, 12 ** -0.5 = 0.289
    assert rr <= 0.5 * rh


def test_pose_seeds_qualify():
    assert len(fr.POSE_SEEDS) == len(set(fr.POSE_SEEDS)) == 8
    for seed in fr.POSE_SEEDS:
        sc, hard, sub = scene(seed, 1.0)
        eh, er = fr.refit_translation_error(sc, hard), fr.refit_translation_error(sc, sub)
        print("seed %d: translation error %.4f m from the hard cells, %.4f m from the refined points, ratio %.2f" % (seed, eh, er, eh / er))
        assert er * 1.5 <= eh, seed


def test_c1_basis_never_gives_a_zero_denominator():
    fmap = fr.feature_map(8, 12, fr.C1_BASIS)[:, 0].reshape(8, 12)
    s = np.sign(fmap)
    assert np.all(s != 0) and np.all(np.abs(fmap) > 0.5)
    assert np.all(s[:, :-2] != s[:, 2:]) and np.all(s[:-2, :] != s[2:, :])      # the two neighbours of a cell differ, on both axes


def test_python_surface():
    from cofii2p_amd import evaluation, ops, pose
    from cofii2p_amd.network import CoFiI2P
    from cofii2p_amd.serving import FrameBatcher

    assert list(inspect.signature(ops.fine_refine).parameters) == ["fmap", "H2", "W2", "coarse_xy", "fine_pc", "best", "count", "center_scale",
                                                                  "frames"]
    for fn in (CoFiI2P.forward_async, FrameBatcher.__init__, evaluation.evaluate):
        assert inspect.signature(fn).parameters["subpixel"].default is False, fn
    # one accessor decides which image points a submission's consumers read
    a, b = object(), object()
    assert pose.image_points([{"fine_xy_all": a}]) is a
    assert pose.image_points([{"fine_xy_all": a, "sub_xy_all": b}]) is b
    fb = FrameBatcher(None, subpixel=True, pose=True)
    assert fb.subpixel and not FrameBatcher(None).subpixel
    with pytest.raises(RuntimeError):
        FrameBatcher(None).sub_xy((0, 0, 0))                                      # built without subpixel=True
