"""The restatements of tests/attention_refs.py without a GPU: float32 against the oracle, the error bound against a plain float32
evaluation and against the emulated six-product split (the two conditions that fix its constants C1 = 2, C2 = 1/8), the mutations the
bound has to catch, the key splits the cases were chosen for, and the layer tail against the oracle's layer.

Largest ratios error / bound over CASES x REGIMES with C1 = 2, C2 = 1/8 (printed per case by the tests below):
    float32 restatement   0.38  (f16-L128-S70-H4, sentinel_up)     limit 0.5
    six-product split     0.28  (f1-L96-S5-H4, flat)               limit 1.0
Smallest mutation ratio on the flat regime: 4.6 (k rounded to its bf16 hi plane at S = 923); every other mutation is above 250.

Mutations that do not apply (mutation_applicable; nothing is skipped silently, test_exemptions_are_these pins the list):
    drop_last_key, k_bf16_hi         S = 1: (1, 1, 1, 4) - no key to drop, and a single key weighs 1 whatever its score
    drop_block, double_block         S <= 32: (1, 1, 1, 4), (1, 31, 32, 4), (1, 32, 31, 4), (1, 96, 5, 4), (1, 64, 27, 4) - one block
    frame_leak                       frames = 1: every case but (3, 40, 50, 4), (2, 33, 257, 4), (16, 128, 70, 4)
"""
import pytest
import torch

import attention_refs as R
import cofi_oracle as O
from common import load_golden

IDS = [R.case_id(c) for c in R.CASES]


def oracle_attention(q, k, v, cs, H):
    L, S = q.shape[0], k.shape[0]
    qq = q if cs is None else q * cs
    return O.full_attention(qq.view(L, H, 32), k.view(S, H, 32), v.view(S, H, 32)).reshape(L, H * 32)


@pytest.mark.parametrize("case", [(1, 65, 129, 4), (3, 40, 50, 4), (1, 70, 100, 8)], ids=R.case_id)
@pytest.mark.parametrize("regime", ["flat", "peaked"])
def test_float32_restatement_equals_the_oracle(case, regime):
    """both are float32 torch with the same operation order: 1e-5 absolute"""
    inp = R.case_inputs(case, regime)
    for f in range(case[0]):
        q, k, v, cs = R.frame_slices(case, inp, f)
        out = R.full_attention(q, k, v, cs, nhead=case[3], dtype=torch.float32)
        assert out.dtype == torch.float32
        d = float((out - oracle_attention(q, k, v, cs, case[3])).abs().max())
        print("%s %s frame %d: max |restatement32 - oracle| = %.3g" % (R.case_id(case), regime, f, d))
        assert d <= 1e-5


@pytest.mark.parametrize("regime", R.REGIMES)
@pytest.mark.parametrize("case", R.CASES, ids=IDS)
def test_float32_and_split_emulation_within_the_bound(case, regime):
    """the two conditions that fix C1 and C2: float32 under half the bound, the emulated split arithmetic under the bound"""
    inp = R.case_inputs(case, regime)
    o64, bound = R.reference_and_bound(case, regime)
    assert bool((bound > 0).all()) and bool(torch.isfinite(bound).all())
    r32 = float(((R.reference(case, inp, torch.float32).double() - o64).abs() / bound).max())
    r6 = float(((R.split6(case, inp).double() - o64).abs() / bound).max())
    print("%-18s %-13s float32 / bound = %.3f   split6 / bound = %.3f" % (R.case_id(case), regime, r32, r6))
    assert r32 <= 0.5
    assert r6 <= 1.0


@pytest.mark.parametrize("case", R.CASES, ids=IDS)
def test_every_applicable_mutation_breaks_the_bound(case):
    """a defect of the kind a kernel can have - a key dropped or counted past S, a block dropped or counted twice, another frame's
    keys, K at bf16 precision - is above the bound on the flat inputs, where every key weighs about 1 / S"""
    inp = R.case_inputs(case, "flat")
    o64, bound = R.reference_and_bound(case, "flat")
    ran = 0
    for kind in R.MUTATIONS:
        if not R.mutation_applicable(case, kind):
            continue
        ratio = float(((R.mutated(case, inp, kind) - o64).abs() / bound).max())
        print("%-18s %-14s mutation / bound = %.4g" % (R.case_id(case), kind, ratio))
        assert ratio > 1.0, kind
        ran += 1
    assert ran >= 1


def test_exemptions_are_these():
    """the not-applicable (case, mutation) pairs, stated: only the single-key case is exempt from a mutation that its shape would allow"""
    na = {kind: [c for c in R.CASES if not R.mutation_applicable(c, kind)] for kind in R.MUTATIONS}
    one_block = [(1, 1, 1, 4), (1, 31, 32, 4), (1, 32, 31, 4), (1, 96, 5, 4), (1, 64, 27, 4)]
    assert na["drop_last_key"] == [(1, 1, 1, 4)] and na["k_bf16_hi"] == [(1, 1, 1, 4)] and na["extra_key"] == []
    assert na["drop_block"] == one_block and na["double_block"] == one_block
    assert [c for c in R.CASES if c not in na["frame_leak"]] == [(3, 40, 50, 4), (2, 33, 257, 4), (16, 128, 70, 4)]
    assert all(c[2] > 32 for c in R.CASES if c not in one_block) and all(c[0] == 1 for c in na["frame_leak"])


def test_key_layout_covers_every_split_on_256_compute_units():
    lays = {c: R.key_layout(c[1], c[2], c[3], c[0], 256) for c in R.CASES}
    for c, lay in lays.items():
        print("%-18s P %2d QB %d QSB %d KS %d light %d ranges %s" % (R.case_id(c), lay["P"], lay["QB"], lay["QSB"], lay["KS"], lay["light"], lay["ranges"]))
        assert lay["KS"] == R.EXPECTED_KS[c], c
        assert sum(n for _, n in lay["ranges"]) == lay["P"] and lay["ranges"][0][0] == 0
        assert all(a[0] + a[1] == b[0] for a, b in zip(lay["ranges"], lay["ranges"][1:]))
    assert {lay["KS"] for lay in lays.values()} == set(range(1, 9))
    assert all(lays[c]["KS"] == ks for ks, c in R.KS_CASES.items())
    assert sum(1 for lay in lays.values() if lay["P"] % lay["KS"]) >= 3
    assert all(lays[c]["P"] % ks for ks, c in R.KS_CASES.items() if ks > 1)                # the KS cases: uneven ranges
    assert any(lay["QB"] % 2 for lay in lays.values())                                      # an idle wave pair
    assert any(lay["light"] == 1 for lay in lays.values()) and any(lay["light"] == 0 for lay in lays.values())
    # a range that ends inside a step (waves without a unit), and one that fills its steps
    assert any(n % R.KPH for lay in lays.values() for _, n in lay["ranges"]) and any(n % R.KPH == 0 for lay in lays.values() for _, n in lay["ranges"])
    # the light case is the smallest: one frame less and the heavy variant runs
    assert R.key_layout(128, 70, 4, 15, 256)["light"] == 0


def test_split_planes_are_exact():
    """hi + mid + lo == x exactly for float32 x (24 mantissa bits in three times 8)"""
    g = torch.Generator().manual_seed(0)
    x = torch.randn(4096, generator=g) * torch.exp(4 * torch.randn(4096, generator=g))
    hi, mid, lo = R.planes3(x)
    assert torch.equal((hi.double() + mid.double() + lo.double()).float(), x)
    assert torch.equal(hi, hi.bfloat16().float()) and torch.equal(lo, lo.bfloat16().float())


def test_layer_tail_float32_equals_the_oracle_layer():
    """layer_tail fed the oracle's own attention output is the rest of O.loftr_layer: 1e-5 absolute"""
    m = load_golden("micro_ops.npz")
    t = lambda a: torch.from_numpy(a)
    x, src = t(m["lay_x"]), t(m["lay_src"])
    w = {n[len("lay_w_"):]: t(m[n]) for n in m.files if n.startswith("lay_w_")}
    L, C = x.shape
    q = x @ w["q_proj.weight"].t()
    q = q / q.norm(dim=0, keepdim=True).clamp_min(1e-12)
    k, v = src @ w["k_proj.weight"].t(), src @ w["v_proj.weight"].t()
    msg = O.full_attention(q.view(L, 4, 32), k.view(-1, 4, 32), v.view(-1, 4, 32)).reshape(L, C)
    res = R.layer_tail(msg, x, w, dtype=torch.float32)
    want = O.loftr_layer({"l." + n: a for n, a in w.items()}, "l.", x, src)
    d = float((res["out"] - want).abs().max())
    print("max |layer_tail32 - oracle layer| = %.3g" % d)
    assert res["out"].dtype == torch.float32 and d <= 1e-5
    assert float((res["out"] - t(m["lay_out"])).abs().max()) <= 1e-5                      # ... and the reference's recorded output
    # the by-products are what they say
    assert torch.allclose(res["l2"].norm(dim=1), torch.ones(L), atol=1e-6)
    assert torch.allclose(res["q"], res["out"] @ w["q_proj.weight"].t())
    y = torch.cat([res["q"], res["k"], res["v"]], 1)
    assert res["part"].shape == ((L + 31) // 32, 3 * C, 2)
    assert torch.allclose(res["part"][:, :, 0].sum(0), y.sum(0), atol=1e-4) and torch.allclose(res["part"][-1, :, 1], (y[32 * (L // 32):] ** 2).sum(0), atol=1e-4)
