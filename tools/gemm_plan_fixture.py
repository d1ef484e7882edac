"""The GEMM planner's answers for a fixed request set (tests/golden/gemm_plans.npz), through cofi_tune_describe_gemm / _conv.  CPU only.

    python -m tools.gemm_plan_fixture --write [--lib PATH]     record the fixture (done ONCE, with the describe hooks laid over the entries of
                                                               the commit before csrc/gemm_planner.h existed; never regenerate it from a later
                                                               planner: a plan that differs from the fixture is a bug in the planner)
    python -m tools.gemm_plan_fixture --check [--env I]        replay the rows of environment state I (0 = no switch set) and count mismatches
    python -m tools.gemm_plan_fixture --invariants [--lib P]   count the planner invariants' violations (tests/test_gemm_plans_cpu.py asserts them)

A request row is (kind, 12 arguments, override state, environment state, group); kind 0 = cofi_tune_describe_gemm(M, N, K, act, fused_ln,
pending_norm, frames, ws_bytes), kind 1 = cofi_tune_describe_conv(H, W, Cin, Cout, ks, stride, pad, ldx, act, pending_norm, frames, ws_bytes).
Override states are rows of STATES (the arguments of the five cofi_tune_* setters), environment states rows of ENVS (read once per process:
one process each).  tests/test_gemm_plans_cpu.py replays the rows it finds in the fixture - it does not regenerate requests."""
import argparse
import ctypes
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from cofii2p_amd import _lib  # noqa: E402

FIXTURE = os.path.join(ROOT, "tests", "golden", "gemm_plans.npz")
CSRC = os.path.join(ROOT, "cofii2p_amd", "csrc")

X3, WS, AS, X6, L2, F16, WF16 = 0x100, 0x200, 0x400, 0x800, 0x1000, 0x2000, 0x4000   # COFI_GEMM_* of include/cofi_hip.h
PLAN_FIELDS = ("status", "family", "bm", "bn", "ksplit", "kchunk", "pcfg", "partial_bytes", "flag_offset", "ws_bytes")
F16_FAMILIES = (5, 6, 7)   # COFI_PLAN_BIG_F16, _W4, _128
GROUPS = ("grid", "tables", "conv", "overrides", "illegal", "env")

# (force_plan bm, bn, ksplit | force_planes cfg, ksplit | force_big mode, ksplit | force_conv_direct mode | big_debug flags)
DEFAULT_STATE = (0, 0, 0, -1, 0, 0, 0, 0, 0)
STATES = [DEFAULT_STATE]
STATES += [(bm, bn, ks, -1, 0, 0, 0, 0, 0) for bm in (64, 128) for bn in (64, 128) for ks in (0, 3)]
STATES += [(0, 0, 0, cfg, ks, 0, 0, 0, 0) for cfg, ks in ((5, 0), (2, 2), (-2, 0))]
STATES += [(0, 0, 0, -1, 0, mode, ks, 0, 0) for mode, ks in ((1, 0), (1, 4), (-1, 0))]
STATES += [(0, 0, 0, -1, 0, 0, 0, mode, 0) for mode in (1, 2, -1)]
STATES += [(0, 0, 0, -1, 0, 0, 0, 0, dbg) for dbg in (256, 512)]

ENVS = [None, ("COFI_GEMM_BIG", "0"), ("COFI_GEMM_TALL_TILE", "0"), ("COFI_GEMM_F16_KS1_TILES", "0"), ("COFI_GEMM_F16_TABLE", "0"),
        ("COFI_GEMM_X6_PLANS", "0"), ("COFI_CONV_DIRECT", "0"), ("COFI_GEMM_F16_BM256", "1")]


def load(path=None):
    lib = ctypes.CDLL(path or _lib.LIB_PATH)
    queries = ("cofi_gemm_f16x3_eligible", "cofi_conv2d_f16x3_eligible", "cofi_gemm_f32_workspace")
    for name, sig in list(_lib.TUNE_SIGNATURES.items()) + [(q, _lib.SIGNATURES[q]) for q in queries]:
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = sig
    return lib


def set_state(lib, st):
    st = [int(v) for v in st]
    rcs = (lib.cofi_tune_force_plan(*st[0:3]), lib.cofi_tune_force_planes(*st[3:5]), lib.cofi_tune_force_big(*st[5:7]),
           lib.cofi_tune_force_conv_direct(st[7]), lib.cofi_tune_big_debug(st[8]))
    assert not any(rcs), (st, rcs)


def describe(lib, kind, args, desc=None):
    desc = desc or _lib.PlanDesc()
    (lib.cofi_tune_describe_conv if kind else lib.cofi_tune_describe_gemm)(*([int(v) for v in args[:12 if kind else 8]] + [ctypes.byref(desc)]))
    return tuple(getattr(desc, f) for f in PLAN_FIELDS)


def replay(lib, req, states):
    """The plans of the request rows `req` (n, 16), under the override state each names; the defaults are restored afterwards."""
    out = np.zeros((len(req), len(PLAN_FIELDS)), np.int64)
    desc = _lib.PlanDesc()
    try:
        for s in np.unique(req[:, 13]):
            set_state(lib, states[s])
            for i in np.nonzero(req[:, 13] == s)[0]:
                out[i] = describe(lib, req[i, 0], req[i, 1:13].tolist(), desc)
    finally:
        set_state(lib, DEFAULT_STATE)
    return out


def load_fixture(path=FIXTURE):
    """-> {"req": (n, 16), "plan": (n, 10), "states": (s, 9)} int64.  The file holds the two tables column by column (it compresses better)."""
    fx = np.load(path)
    return {"req": np.ascontiguousarray(fx["req"].T), "plan": np.ascontiguousarray(fx["plan"].T), "states": fx["states"]}


def save(path, fx):
    np.savez_compressed(path, req=np.ascontiguousarray(fx["req"].T), plan=np.ascontiguousarray(fx["plan"].T), states=fx["states"])


# ---- the request set
def table_shapes():
    shapes = []
    for name in ("gemm_plans.inc", "gemm_plans_x6.inc", "gemm_plans_big.inc", "gemm_planes_plans.inc"):
        for m in re.finditer(r"^\s*\{\s*(\d+),\s*(\d+),\s*(\d+),", open(os.path.join(CSRC, name)).read(), flags=re.M):
            s = tuple(int(v) for v in m.groups())
            if s[0] > 0 and s not in shapes:
                shapes.append(s)
    return shapes


def conv_mnk(a):
    H, W, Cin, Cout, ks, stride, pad = a[:7]
    if stride <= 0:
        return 0, 0, 0
    return ((H + 2 * pad - ks) // stride + 1) * ((W + 2 * pad - ks) // stride + 1) * a[10], Cout, ks * ks * Cin


def gemm_forms(N):
    """(act, fused_ln, pending_norm, frames): every legal flag combination"""
    base = [0, X3, X3 | WS, X3 | WS | AS, X6, X6 | WS, X6 | F16, X6 | F16 | WF16, X3 | F16, X6 | 2]
    forms = [(a, 0, 0, 1) for a in base]
    norm = [X3 | WS, X6, X6 | WS, X6 | F16, X6 | F16 | WF16]
    if N <= 128:
        forms += [(a | L2, 0, 0, 1) for a in (0, X3, X3 | WS, X6, X6 | WS, X6 | F16)]
        forms += [(a, 1, 0, 1) for a in (0, X3 | 1, X3 | WS, X6, X6 | WS | 1)]
        norm = norm + [X6 | L2]
    forms += [(a, 0, 1, f) for a in norm for f in (1, 16)]
    return forms


ILLEGAL = [(WF16, 0, 0, 1), (X6 | F16 | WF16 | WS, 0, 0, 1), (WS, 0, 0, 1), (X6 | AS, 0, 0, 1), (X6 | WS | AS, 0, 0, 1), (X3 | AS, 0, 0, 1),
           (X3 | 5, 0, 0, 1), (X3 | WS | AS | L2, 0, 0, 1), (X3 | L2, 0, 0, 1), (0, 0, 1, 1), (X3, 0, 1, 16), (X6, 0, 0, 0), (X3 | WS | AS, 0, 1, 1),
           (WS, 1, 0, 1), (X6 | WS | L2 | 7, 0, 0, 1)]


def generate(lib):
    """-> req (n, 16) int64: kind, 12 arguments (ws_bytes resolved against `lib`; a dense request uses the first 8), state, env, group"""
    rows = []

    def add(kind, args, state, env, group):
        """the request with the query's workspace, with none, and one byte short of its plan's flags / partials"""
        set_state(lib, STATES[state])
        mnk = conv_mnk(args) if kind else args[:3]
        wsq = lib.cofi_gemm_f32_workspace(*mnk) if min(mnk) > 0 else 0
        p = dict(zip(PLAN_FIELDS, describe(lib, kind, list(args) + [wsq])))
        sizes = [wsq]
        if group < 3 and p["status"] == 0 and p["ws_bytes"] > 0:   # (override and environment states: the query's workspace only)
            sizes += [0, p["ws_bytes"] - 1] + ([p["partial_bytes"] - 1] if 0 < p["partial_bytes"] < p["ws_bytes"] else [])
        for ws in sizes:
            rows.append([kind] + list(args) + [ws] + [0] * (11 - len(args)) + [state, env, group])

    def gemm(M, N, K, state, env, group, forms=None):
        for act, ln, pn, fr in forms or gemm_forms(N):
            add(0, [M, N, K, act, ln, pn, fr], state, env, group)

    tables = table_shapes()
    # a grid around the thresholds of the code; rows per frame (frames = 16) that are / are not multiples of 128 and 256: 6144 = 16 * 384
    for M in (1, 63, 64, 65, 255, 256, 257, 1280, 5120, 6144, 20480, 81920, 327680):
        for N in (4, 32, 33, 64, 65, 128, 129, 256, 512, 1024):
            for K in (4, 28, 32, 64, 128, 252, 256, 508, 512, 516, 576, 1024, 1152, 2304, 7680):
                gemm(M, N, K, 0, 0, 0)
    # every shape of the four tuned tables, with its neighbours
    for M0, N, K in tables:
        for M in sorted({M0, M0 - 1, M0 + 1, 2 * M0, M0 // 2}):
            if M >= 1:
                gemm(M, N, K, 0, 0, 1)
    # convolutions
    conv_acts = [0, X3, X3 | WS, X6, X6 | WS, X6 | F16, X6 | F16 | WF16]
    conv_norm_acts = [X3 | WS, X6, X6 | F16, X6 | F16 | WF16]

    def conv(H, W, Cin, Cout, ks, stride, pad, ldx, frames, state, env, group):
        if (H + 2 * pad - ks) // stride + 1 <= 0 or (W + 2 * pad - ks) // stride + 1 <= 0:
            return   # no output pixels: nothing the entries plan
        for act in conv_acts + ([X6 | L2] if Cout <= 128 else []):
            add(1, [H, W, Cin, Cout, ks, stride, pad, ldx, act, 0, frames], state, env, group)
        for pn in (1, 2):
            for act in conv_norm_acts:
                add(1, [H, W, Cin, Cout, ks, stride, pad, ldx, act, pn, frames], state, env, group)

    maps = ((5, 1), (4, 64), (8, 128), (40, 128), (160, 512))
    for ks in (1, 3):
        for stride in (1, 2):
            for pad in (0, 1):
                for Cin in (4, 16, 32, 48, 64, 512, 528):
                    for Cout in (32, 64, 128, 256):
                        for H, W in maps:
                            for frames in (1, 16):
                                for ldx in (Cin, Cin + 8) if (Cin in (32, 64) and ks == 3) else (Cin,):
                                    conv(H, W, Cin, Cout, ks, stride, pad, ldx, frames, 0, 0, 2)
    # every override state on a sub-grid
    for state in range(1, len(STATES)):
        for M in (256, 1280, 20480, 81920):
            for N in (64, 128, 256):
                for K in (128, 512, 1152, 2304):
                    gemm(M, N, K, state, 0, 3)
        for Cin in (16, 32, 64):
            for Cout in (64, 128):
                for H, W in maps[2:]:
                    for frames in (1, 16):
                        conv(H, W, Cin, Cout, 3, 1, 1, Cin, frames, state, 0, 3)
    # illegal combinations, for their status codes
    for M, N, K in ((1280, 64, 512), (20480, 256, 1152)):
        gemm(M, N, K, 0, 0, 4, ILLEGAL)
    for act, pn, fr in ((WF16, 0, 1), (WS, 0, 1), (X6 | AS, 0, 1), (X6 | 4, 0, 1), (X6 | L2, 0, 1), (X3, 1, 1), (X6, 0, 0)):
        add(1, [40, 128, 64, 256, 3, 1, 1, 64, act, pn, fr], 0, 0, 4)
    add(1, [40, 128, 64, 256, 2, 1, 1, 64, X6, 0, 1], 0, 0, 4)
    add(1, [40, 128, 64, 256, 3, 0, 1, 64, X6, 0, 1], 0, 0, 4)
    set_state(lib, DEFAULT_STATE)
    # each environment switch, in a process of its own: the table shapes as listed, and the convolutions the switches touch.  The workspace
    # sizes are those of the unswitched library (the rows are resolved here, in one process).
    base = len(rows)
    for M, N, K in tables:
        gemm(M, N, K, 0, 0, 5)
    for Cin in (32, 64):
        for Cout in (64, 256):
            for H, W in maps[2:]:
                conv(H, W, Cin, Cout, 3, 1, 1, Cin, 16, 0, 0, 5)
    env_rows = rows[base:]
    del rows[base:]
    for e in range(1, len(ENVS)):
        rows += [r[:14] + [e, 5] for r in env_rows]
    return np.asarray(rows, np.int64)


# ---- the invariants one planner behind entries and queries makes true
def invariants(lib, req, plans, states):
    """-> {name: indices of the rows that violate it}.  Evaluated under each row's override state; rows of environment state 0 only."""
    bad = {"eligible_is_the_plan": [], "workspace_covers_plan": [], "presplit_eligible_runs": [], "flags_behind_partials": []}
    desc = _lib.PlanDesc()
    try:
        for s in np.unique(req[:, 13]):
            set_state(lib, states[s])
            for i in np.nonzero((req[:, 13] == s) & (req[:, 14] == 0))[0]:
                kind, a, p = req[i, 0], req[i, 1:13].tolist(), dict(zip(PLAN_FIELDS, plans[i].tolist()))
                M, N, K = conv_mnk(a) if kind else a[:3]
                act, pn, fr, ws = (a[8], a[9], a[10], a[11]) if kind else (a[3], a[5], a[6], a[7])
                wsq = lib.cofi_gemm_f32_workspace(M, N, K) if min(M, N, K) > 0 else 0
                elig = lib.cofi_conv2d_f16x3_eligible(*(a[:8] + [pn, fr])) if kind else lib.cofi_gemm_f16x3_eligible(M, N, K, pn, fr)
                if p["status"] == 0 and p["ws_bytes"] > wsq:
                    bad["workspace_covers_plan"].append(i)
                if act & ~3 == X6 | F16 and ws == wsq and not (kind == 0 and a[4]) and (elig == 1) != (p["status"] == 0 and p["family"] in F16_FAMILIES):
                    bad["eligible_is_the_plan"].append(i)
                if act & WF16 and act & ~3 == X6 | F16 | WF16 and ws == wsq and elig == 1 and p["status"] != 0:
                    bad["presplit_eligible_runs"].append(i)
                if p["status"] == 0 and p["flag_offset"] >= 0:
                    words = -(-M // p["bm"]) * -(-N // p["bn"]) * p["ksplit"]   # one per workgroup of the launch
                    if p["flag_offset"] < p["partial_bytes"] or p["flag_offset"] + 4 * words > p["ws_bytes"] or p["ws_bytes"] > ws:
                        bad["flags_behind_partials"].append(i)
    finally:
        set_state(lib, DEFAULT_STATE)
    return {k: np.asarray(v, np.int64) for k, v in bad.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--write", action="store_true")
    ap.add_argument("--check", action="store_true")
    ap.add_argument("--invariants", action="store_true")
    ap.add_argument("--env", type=int, default=0)
    ap.add_argument("--lib", default=None)
    ap.add_argument("--fixture", default=FIXTURE)
    a = ap.parse_args()
    if a.env:
        assert os.environ.get(ENVS[a.env][0]) == ENVS[a.env][1], "start this process with %s=%s" % ENVS[a.env]
    lib = load(a.lib)
    if a.write:
        if a.env:   # second pass, one process per switch: fill in the plans of that environment state
            fx = load_fixture(a.fixture)
            sel = fx["req"][:, 14] == a.env
            fx["plan"][sel] = replay(lib, fx["req"][sel], fx["states"])
        else:
            req = generate(lib)
            fx = {"req": req, "states": np.asarray(STATES, np.int64), "plan": np.zeros((len(req), len(PLAN_FIELDS)), np.int64)}
            sel = req[:, 14] == 0
            fx["plan"][sel] = replay(lib, req[sel], fx["states"])
        save(a.fixture, fx)
        print("wrote %d rows (%d of environment state %d) to %s" % (len(fx["req"]), int(sel.sum()), a.env, a.fixture))
        return 0
    fx = load_fixture(a.fixture)
    req, plan, states = fx["req"], fx["plan"], fx["states"]
    if a.check:
        sel = req[:, 14] == a.env
        got = replay(lib, req[sel], states)
        wrong = np.nonzero((got != plan[sel]).any(axis=1))[0]
        for i in wrong[:10]:
            print("request", req[sel][i].tolist(), "fixture", plan[sel][i].tolist(), "planner", got[i].tolist())
        print("environment state %d (%s): %d rows, %d differ" % (a.env, ENVS[a.env], int(sel.sum()), len(wrong)))
        return 1 if len(wrong) else 0
    if a.invariants:
        sel = req[:, 14] == 0
        got = replay(lib, req[sel], states)
        for k, v in invariants(lib, req[sel], got, states).items():
            print("%s: %d of %d rows violate it" % (k, len(v), int(sel.sum())))
            for i in v[:8]:
                print("   request", req[sel][i].tolist(), "plan", got[i].tolist())
    return 0


if __name__ == "__main__":
    sys.exit(main())
