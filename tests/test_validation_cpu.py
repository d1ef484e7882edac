"""Host side of the validation pass (cofii2p_amd.validation) against tests/golden/val_ref.npz, the reference's own `test_acc`
(train.py:27-106) on six tiny frames (tests/tools/make_golden_val.py).  No GPU needed."""
import numpy as np
import torch

from common import load_golden


def _gold():
    return load_golden("val_ref.npz")


def counting_rule(dist: torch.Tensor, mask: torch.Tensor, topk: int = 5):
    """train.py:89-101 restated without its Python loops: the true set = values of dist where mask is set and mask * dist != 0; per row
    the topk smallest values ascending; counts[k - 1] = candidates among the first k of every row whose VALUE is in the true set."""
    true_vals = dist[(mask * dist) != 0]
    cand = torch.sort(dist, dim=-1).values[:, :topk]                                   # (K, topk)
    member = (cand[:, :, None] == true_vals[None, None, :]).any(-1)                    # (K, topk)
    return torch.cumsum(member.sum(0), 0).to(torch.int32), int(true_vals.numel())


def test_fixture_is_data_and_holds_duplicates():
    g = _gold()
    assert all(g[k].dtype.kind in "fiuUb" for k in g.files)                            # numbers and hash strings, no objects
    B, K = len(g["frame_ids"]), int(g["num_kpt"])
    assert B == 6 and g["counts"].shape == (6, 5) and g["n_true"].shape == (6,) and g["fine_hits"].shape == (6,) and g["score_stats"].shape == (6, 6)
    assert any(len(np.unique(g["lab%d_pc_kpt_idx" % f])) < K for f in range(B))       # sampling with replacement: membership by value matters


def test_reference_acc_reproduces_test_acc():
    from cofii2p_amd.validation import frame_recall, reference_acc

    g = _gold()
    counts, n_true = torch.from_numpy(g["counts"]), torch.from_numpy(g["n_true"])
    assert torch.equal(reference_acc(counts, n_true), torch.from_numpy(g["acc"]))
    assert torch.equal(reference_acc(counts[:3], n_true[:3]), torch.from_numpy(g["acc3"]))   # 3 frames: still averaged over 6 rows
    assert torch.equal(reference_acc(counts[:3], n_true[:3]), reference_acc(torch.cat([counts[:3], counts[:3] * 0]), n_true[[0, 1, 2, 0, 1, 2]]))   # missing rows = zero rows
    assert torch.equal(reference_acc(torch.cat([counts, counts]), torch.cat([n_true, n_true * 0])), torch.from_numpy(g["acc"]))                # frames past the sixth are never read
    # a last frame without a true pair: torch's division (train.py:103 divides a tensor by the python int 0)
    n0 = n_true.clone()
    n0[5] = 0
    c0 = counts.clone() + 1
    c0[:, 0] = 0
    want = torch.mean(c0.float() / 0, dim=0)
    got = reference_acc(c0, n0)
    assert torch.isnan(want[0]) and torch.isinf(want[4])
    assert torch.equal(torch.isnan(got), torch.isnan(want)) and torch.equal(got[~torch.isnan(got)], want[~torch.isnan(want)])
    # the per-frame recall divides every frame by its own number of true pairs
    rec = frame_recall(counts, n_true)
    assert rec.shape == (6, 5) and torch.equal(rec, counts.float() / n_true.float()[:, None])
    assert torch.equal(rec[5] * 1, counts[5].float() / float(n_true[5]))


def test_counting_rule_restatement_agrees_with_the_fixture():
    g = _gold()
    for f in range(6):
        c, n = counting_rule(torch.from_numpy(g["dist_%d" % f]), torch.from_numpy(g["mask_%d" % f]))
        assert n == int(g["n_true"][f]), f
        assert torch.equal(c, torch.from_numpy(g["counts"][f])), (f, c, g["counts"][f])


def test_header_and_binding_declare_the_validation_entry_points():
    from cofii2p_amd import _lib

    names = set(_lib.header_symbols())
    assert {"cofi_val_monitors", "cofi_val_monitors_workspace", "cofi_val_gather"} <= names
    assert names == set(_lib.SIGNATURES)
    res, args = _lib.SIGNATURES["cofi_val_monitors"]
    assert res is _lib.c_int and len(args) == 32 and args[-1] is _lib.c_void_p
    assert _lib.SIGNATURES["cofi_val_monitors_workspace"] == (_lib.c_size_t, [_lib.c_int, _lib.c_int])
