"""The GEMM planner (csrc/gemm_planner.h) against tests/golden/gemm_plans.npz: every plan of a fixed request set - family, tile, K split,
partials, flag offset, workspace, status - equals the plan the entries made before the planner existed (the fixture was recorded once, with
the describe hooks laid over those entries; tools/gemm_plan_fixture.py).  Host arithmetic only: no GPU.

A mismatch is a bug in the planner.  The fixture is never regenerated from the code under test."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tools import gemm_plan_fixture as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    return G.load()


@pytest.fixture(scope="module")
def fx():
    return G.load_fixture()


def test_request_set_covers_what_it_must(fx):
    """The fixture is only as good as its requests: every table shape, the threshold grid, every override and environment state."""
    req, states = fx["req"], fx["states"]
    dense = req[req[:, 0] == 0]
    have = {tuple(r) for r in dense[:, 1:4].tolist()}
    for M, N, K in G.table_shapes():
        for m in (M, M - 1, M + 1, 2 * M, M // 2):
            assert (m, N, K) in have, (m, N, K)
    assert {(M, N, K) for M in (1, 63, 64, 65, 255, 256, 257, 1280, 5120, 20480, 81920, 327680) for N in (4, 32, 33, 64, 65, 128, 129, 256, 512, 1024)
            for K in (4, 28, 32, 64, 128, 252, 256, 508, 512, 516, 576, 1024, 1152, 2304, 7680)} <= have
    assert states.tolist() == [list(s) for s in G.STATES] and set(req[:, 13].tolist()) == set(range(len(G.STATES)))
    assert set(req[:, 14].tolist()) == set(range(len(G.ENVS)))
    conv = req[req[:, 0] == 1]
    for col, values in ((5, (1, 3)), (6, (1, 2)), (7, (0, 1)), (3, (4, 16, 32, 48, 64, 512, 528)), (4, (32, 64, 128, 256)), (10, (0, 1, 2)), (11, (1, 16))):
        assert set(values) <= set(conv[:, col].tolist()), (col, values)
    assert (conv[:, 8] > conv[:, 3]).any()   # an ldx larger than Cin
    assert (fx["plan"][:, 0] != 0).any() and len(req) == len(fx["plan"])


@pytest.mark.parametrize("group", [g for g in G.GROUPS if g != "env"])
def test_plans_equal_the_fixture(lib, fx, group):
    sel = (fx["req"][:, 15] == G.GROUPS.index(group)) & (fx["req"][:, 14] == 0)
    assert sel.any()
    try:
        got = G.replay(lib, fx["req"][sel], fx["states"])
    finally:
        G.set_state(lib, G.DEFAULT_STATE)
    wrong = np.nonzero((got != fx["plan"][sel]).any(axis=1))[0]
    assert len(wrong) == 0, "%d of %d plans differ; first: request %s fixture %s planner %s" % (
        len(wrong), int(sel.sum()), fx["req"][sel][wrong[0]].tolist(), fx["plan"][sel][wrong[0]].tolist(), got[wrong[0]].tolist())


def test_environment_switches_equal_the_fixture(fx):
    """Each switch is read once per process: one child per switch (started together), over the tables' shapes."""
    children = []
    for e in range(1, len(G.ENVS)):
        assert (fx["req"][:, 14] == e).any()
        env = dict(os.environ)
        env[G.ENVS[e][0]] = G.ENVS[e][1]
        children.append((e, subprocess.Popen([sys.executable, "-m", "tools.gemm_plan_fixture", "--check", "--env", str(e)], cwd=ROOT, env=env,
                                             stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)))
    for e, child in children:
        out = child.communicate()[0]
        assert child.returncode == 0 and "0 differ" in out, (G.ENVS[e], out[-2000:])


def test_invariants_of_one_planner(lib, fx):
    """What entries and queries answering from the same planner makes true, over every request of environment state 0 (no exclusions):
    - cofi_gemm_f16x3_eligible / cofi_conv2d_f16x3_eligible == 1 exactly when the plan of the f16 request, given cofi_gemm_f32_workspace
      bytes, is an f16x3 family;
    - a request that plans takes no more workspace than cofi_gemm_f32_workspace(M, N, K), under the same overrides;
    - a pre-split weight (COFI_GEMM_W_F16PRE) whose query said eligible plans with status 0;
    - the flag table starts at or after the end of the partials and ends inside the plan's workspace bytes, which fit the workspace on offer.
    The entries before the planner broke the first and the third for 38 shapes each (a pending norm over 16 frames with M not a multiple of
    16: the restated query said eligible, the entry COFI_EUNSUPPORTED); the plans of those requests are in the fixture and unchanged."""
    sel = fx["req"][:, 14] == 0
    try:
        bad = G.invariants(lib, fx["req"][sel], fx["plan"][sel], fx["states"])
    finally:
        G.set_state(lib, G.DEFAULT_STATE)
    for name, rows in bad.items():
        assert len(rows) == 0, (name, len(rows), fx["req"][sel][rows[:5]].tolist())
