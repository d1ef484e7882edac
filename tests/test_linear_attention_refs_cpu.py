"""Linear attention without a GPU: the torch restatement (tests/linear_attention_refs.py) against the reference's recorded outputs
(tests/golden/linear_attention_micro.npz, made by tests/tools/make_golden_linear.py), and the host side of the feature - C ABI,
binding table, constructor argument."""
import re

import pytest
import torch

import linear_attention_refs as R
from common import load_golden


@pytest.fixture(scope="module")
def micro():
    m, lin = load_golden("micro_ops.npz"), load_golden("linear_attention_micro.npz")
    t = lambda a: torch.from_numpy(a)
    return {"q": t(m["att_q"]).reshape(48, 128), "k": t(m["att_k"]).reshape(80, 128), "v": t(m["att_v"]).reshape(80, 128),
            "x": t(m["lay_x"]), "src": t(m["lay_src"]), "w": {n[len("lay_w_"):]: t(m[n]) for n in m.files if n.startswith("lay_w_")},
            "lin_out": t(lin["lin_out"]), "lay_out": t(lin["lay_out"])}


def test_float32_restatement_equals_the_reference(micro):
    """Both are float32 torch with the same operation order: 1e-5 absolute."""
    out = R.linear_attention(micro["q"], micro["k"], micro["v"], dtype=torch.float32)
    assert out.dtype == torch.float32
    d = float((out - micro["lin_out"]).abs().max())
    print("operator: max |restatement32 - reference| = %.3g" % d)
    assert d <= 1e-5
    lay = R.loftr_layer(micro["w"], micro["x"], micro["src"], dtype=torch.float32)
    d = float((lay - micro["lay_out"]).abs().max())
    print("layer: max |restatement32 - reference| = %.3g" % d)
    assert d <= 1e-5


@pytest.mark.parametrize("L,S", R.CASES)
def test_float32_restatement_within_the_kernel_bound_of_float64(L, S):
    q, k, v = R.case_inputs(L, S)
    cs = R.col_scale(q)
    o64 = R.linear_attention(q, k, v, cs, dtype=torch.float64)
    o32 = R.linear_attention(q, k, v, cs, dtype=torch.float32)
    bound = R.error_bound(q, k, v, cs)
    ratio = float(((o32.double() - o64).abs() / bound).max())
    print("(%d, %d): float32 torch error / bound = %.3g" % (L, S, ratio))
    assert ratio <= 1.0


def test_header_declares_both_entry_points():
    from cofii2p_amd import _lib

    text = re.sub(r"/\*.*?\*/", "", open(_lib.HEADER_PATH).read(), flags=re.S)
    assert re.search(r"size_t\s+cofi_linear_attention_workspace\s*\(\s*int L, int S, int H, int D, int frames\s*\)\s*;", text)
    m = re.search(r"int\s+cofi_linear_attention\s*\(([^;]*)\)\s*;", text)
    assert m is not None
    args = [a.strip() for a in m.group(1).replace("\n", " ").split(",")]
    assert len(args) == 18 and args[0] == "const float *Q" and args[-1] == "cofi_stream_t stream"
    assert {"cofi_linear_attention_workspace", "cofi_linear_attention"} <= set(_lib.header_symbols())


def test_binding_table_has_both_rows_and_abi_is_3():
    from cofii2p_amd import _lib

    assert _lib.ABI_VERSION == 3
    res, args = _lib.SIGNATURES["cofi_linear_attention_workspace"]
    assert res is _lib.c_size_t and len(args) == 5
    res, args = _lib.SIGNATURES["cofi_linear_attention"]
    assert res is _lib.c_int and len(args) == 18
    assert "#define COFI_ABI_VERSION 3" in open(_lib.HEADER_PATH).read()


def test_constructor_refuses_unknown_attention_kinds():
    from cofii2p_amd.network import CoFiI2P

    class Opt:
        img_H, img_W, img_fine_resolution_scale, norm = 160, 512, 32, "gn"

    class OptLinear(Opt):
        attention = "linear"

    with pytest.raises(ValueError):
        CoFiI2P(Opt(), attention="nonsense")

    class OptBad(Opt):
        attention = "nonsense"

    with pytest.raises(ValueError):
        CoFiI2P(OptBad())
    assert CoFiI2P(Opt()).attention == "full"
    assert CoFiI2P(OptLinear()).attention == "linear"
    assert CoFiI2P(Opt(), attention="linear").attention == "linear"
    from model.network import CoFiI2P as Shim

    m = Shim(OptLinear())
    assert m.attention == "linear" and list(m.state_dict()) == list(CoFiI2P(Opt()).state_dict())
