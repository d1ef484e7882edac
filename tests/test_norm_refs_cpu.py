"""The float64 references of tests/norm_refs.py against torch.nn.functional and the CPU oracle on the forms those can express, the fp32
row-sum emulation against a scalar loop, and the operand validation of the normalisation wrappers (cofii2p_amd/ops.py: tensor metadata
only, so it runs here on CPU tensors).  No GPU needed."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import cofi_oracle as O
import norm_refs as R
from common import load_golden


def rn(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


@pytest.mark.parametrize("M,C", [(1, 4), (5, 260), (37, 2048)])
def test_layer_norm_act_reference(M, C):
    x, ga, be, r = rn(M, C, seed=1) * 3 + 1, rn(C, seed=2), rn(C, seed=3), rn(M, C, seed=4)
    ln = F.layer_norm(x, (C,), ga, be, 1e-5)
    tol = dict(rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(R.layer_norm_act(x, ga, be), ln, **tol)
    torch.testing.assert_close(R.layer_norm_act(x, ga, be, slope=0.0), torch.relu(ln), **tol)
    torch.testing.assert_close(R.layer_norm_act(x, ga, be, slope=0.1, res=r, res_first=True), F.leaky_relu(ln + r, 0.1), **tol)
    torch.testing.assert_close(R.layer_norm_act(x, ga, be, slope=0.0, res=r, res_first=False), torch.relu(ln) + r, **tol)


@pytest.mark.parametrize("frames,Mf,C,groups", [(1, 5, 36, 9), (3, 7, 64, 1), (2, 1, 12, 12), (1, 130, 192, 2)])
def test_group_norm_reference(frames, Mf, C, groups):
    x, ga, be, r = rn(frames * Mf, C, seed=5) * 2 + 0.7, rn(C, seed=6), rn(C, seed=7), rn(frames * Mf, C, seed=8)
    mean, rstd = R.group_stats(x, groups, 1e-5, frames)
    # F.group_norm normalises (N, C, *): one frame = one sample with its rows as the spatial axis
    gn = lambda t, g, b: F.group_norm(t.reshape(frames, Mf, C).transpose(1, 2), groups, g, b, 1e-5).transpose(1, 2).reshape(frames * Mf, C)
    tol = dict(rtol=1e-11, atol=1e-11)
    torch.testing.assert_close(R.group_norm_apply(x, (mean, rstd), ga, be, frames=frames), gn(x, ga, be), **tol)
    torch.testing.assert_close(R.group_norm_apply(x, (mean, rstd), frames=frames), gn(x, None, None), **tol)
    packed = torch.stack([mean, rstd], -1)            # the layout ops.group_stats returns
    torch.testing.assert_close(R.group_norm_apply(x, packed, ga, be, slope=0.1, res=r, frames=frames), F.leaky_relu(gn(x, ga, be) + r, 0.1), **tol)
    rs = R.group_stats(r, groups, 1e-5, frames)
    torch.testing.assert_close(R.group_norm_apply(x, packed, ga, be, slope=0.0, res=r, res_stats=rs, res_gamma=be, res_beta=ga, frames=frames),
                               torch.relu(gn(x, ga, be) + gn(r, be, ga)), **tol)
    torch.testing.assert_close(R.group_norm_apply(x, packed, slope=1.0, res=r, res_stats=rs, frames=frames), gn(x, None, None) + gn(r, None, None),
                               **tol)


def test_pos_sine_reference_on_the_golden_inputs():
    mg = load_golden("micro_ops.npz")
    for key in ("pe_grid", "pe_xyz"):
        c = torch.from_numpy(np.ascontiguousarray(mg[key]))
        ref, amax = R.pos_sine(c, 128)
        want = O.pos_sine(c.float(), 128).double()    # fp32: three roundings of the angle, one of the function
        assert ref.shape == want.shape
        assert float((ref - want).abs().max()) <= amax * 2.0 ** -22 + 2.0 ** -22
        n_dim = c.shape[1]
        assert torch.equal(ref[:, n_dim * (128 // n_dim // 2 * 2):], torch.zeros(c.shape[0], 128 - n_dim * (128 // n_dim // 2 * 2), dtype=torch.float64))


def test_row_and_column_references():
    x = rn(37, 65, seed=9)
    x[3] = 0
    torch.testing.assert_close(R.l2norm_rows(x), F.normalize(x, dim=1), rtol=1e-13, atol=0)
    assert torch.equal(R.l2norm_rows(x)[3], torch.zeros(65, dtype=torch.float64))
    torch.testing.assert_close(R.col_inv_norm(x), 1.0 / x.norm(dim=0).clamp_min(1e-12), rtol=1e-13, atol=0)
    assert float(R.col_inv_norm(torch.zeros(4, 2))[0]) == 1e12
    torch.testing.assert_close(R.col_mean(rn(12, 5, seed=10), 3), rn(12, 5, seed=10).reshape(3, 4, 5).mean(1), rtol=1e-13, atol=0)


@pytest.mark.parametrize("C", [4, 8, 32])
def test_row_sum_tree_is_the_butterfly_of_the_kernel(C):
    """scalar fp32 replay of gn_apply_rows: chunk sums (v0 + v1) + (v2 + v3), then rs[l] += rs[l ^ o] for o = 1, 2, 4 ... over the C / 4
    lanes of the row; lane 0 holds the flag's sum"""
    y = (rn(9, C, seed=C) * 3).float()
    y[0] = torch.tensor([1e8, 1.0, -1e8, 1.0] * (C // 4))   # order-sensitive: (1e8 + 1) + (-1e8 + 1) = 0 in fp32, 2 in exact arithmetic
    got = R.row_sum_tree_f32(y)
    f = np.float32
    for m in range(y.shape[0]):
        v = y[m].numpy()
        rs = [f(f(v[4 * l] + v[4 * l + 1]) + f(v[4 * l + 2] + v[4 * l + 3])) for l in range(C // 4)]
        o = 1
        while o < C // 4:
            rs = [f(rs[l] + rs[l ^ o]) for l in range(C // 4)]
            o <<= 1
        assert got[m].numpy().tobytes() == rs[0].tobytes(), m
    assert float(got[0]) == 0.0


# ---------------------------------------------------------------------------------------------------------------- wrapper validation
def _operands(M=6, C=8, frames=1, groups=2):
    z = torch.zeros
    return dict(x=z(M, C), gamma=z(C), beta=z(C), res=z(M, C), res_gamma=z(C), res_beta=z(C), stats=z(groups, 2) if frames == 1 else z(frames, groups, 2),
                res_stats=z(groups, 2) if frames == 1 else z(frames, groups, 2), out=z(M, C))


def _check(ops, frames=1, **kw):
    x = kw.pop("x")
    ops._norm_operands("test", x, frames, **kw)


@pytest.fixture(scope="module")
def ops():
    from cofii2p_amd import ops as _ops

    return _ops


def test_validation_accepts_what_the_kernels_take(ops):
    _check(ops, **_operands())
    _check(ops, frames=3, **_operands(frames=3))
    _check(ops, x=torch.zeros(6, 8))                                    # everything optional
    wide = torch.zeros(6, 24)
    op = _operands()
    op.update(x=wide[:, 4:12], res=wide[:, 12:20], out=wide[:, 16:24])  # column blocks of a wider buffer
    _check(ops, **op)
    one = _operands(M=1)
    one["res"] = torch.zeros(3, 8)[1:2]                                 # a single row: its row stride is never used
    _check(ops, **one)


@pytest.mark.parametrize("name,bad", [
    ("gamma", lambda: torch.zeros(9)), ("gamma", lambda: torch.zeros(7)), ("beta", lambda: torch.zeros(16)[::2]),
    ("beta", lambda: torch.zeros(8, dtype=torch.float64)), ("res_gamma", lambda: torch.zeros(12)), ("res_beta", lambda: torch.zeros(4)),
    ("res", lambda: torch.zeros(6, 12)), ("res", lambda: torch.zeros(7, 8)), ("res", lambda: torch.zeros(5, 8)), ("res", lambda: torch.zeros(8, 6).t()),
    ("res", lambda: torch.zeros(6, 8, dtype=torch.float16)), ("res", lambda: torch.zeros(48)),
    ("out", lambda: torch.zeros(6, 4)), ("out", lambda: torch.zeros(6, 16)[:, ::2]), ("out", lambda: torch.zeros(12, 8)),
    ("stats", lambda: torch.zeros(3, 2)), ("stats", lambda: torch.zeros(2, 3)), ("stats", lambda: torch.zeros(2, 2, 2)),
    ("stats", lambda: torch.zeros(2, 4)[:, :2]), ("stats", lambda: torch.zeros(2, 2, dtype=torch.float64)), ("stats", lambda: torch.zeros(4)),
    ("res_stats", lambda: torch.zeros(1, 2)), ("res_stats", lambda: torch.zeros(4, 2)),
])
def test_validation_refuses_operands_the_kernels_would_overrun(ops, name, bad):
    from cofii2p_amd._lib import CofiError

    op = _operands()
    op[name] = bad()
    with pytest.raises(CofiError, match=name):
        _check(ops, **op)


def test_validation_counts_the_frames_of_the_statistics(ops):
    from cofii2p_amd._lib import CofiError

    op = _operands(frames=3)
    with pytest.raises(CofiError, match="stats"):
        _check(ops, frames=2, **op)
    op = _operands()
    with pytest.raises(CofiError, match="stats"):
        _check(ops, frames=3, **op)


@pytest.mark.parametrize("name", ["gamma", "beta", "res", "res_gamma", "res_beta", "stats", "res_stats", "out"])
def test_validation_refuses_another_device(ops, name):
    """the only place the device refusal is tested: an operand on the `meta` device (no storage) next to a CPU x"""
    from cofii2p_amd._lib import CofiError

    op = _operands()
    op[name] = op[name].to("meta")
    with pytest.raises(CofiError, match=name):
        _check(ops, **op)


def test_wrappers_refuse_host_tensors(ops):
    from cofii2p_amd._lib import CofiError

    # the check every wrapper applies to its primary operand (and, with device=None, _vec to a vector); asked directly, so that
    # this file needs no built library
    x, v = torch.zeros(4, 8), torch.zeros(8)
    with pytest.raises(CofiError, match="CUDA"):
        ops._mat(x, "x")
    with pytest.raises(CofiError, match="CUDA"):
        ops._vec(v, "gamma", 8)
    with pytest.raises(CofiError, match="CUDA"):
        ops._mat(x.to("meta"), "x")


def test_transpose_destination_validation(ops):
    from cofii2p_amd._lib import CofiError

    cpu = torch.device("cpu")
    ops._transpose_out(torch.zeros(8, 6), cpu, 1, 8, 6)
    ops._transpose_out(torch.zeros(8, 10)[:, :6], cpu, 1, 8, 6)            # ldy > M
    ops._transpose_out(torch.zeros(3, 8, 6), cpu, 3, 8, 6)
    ops._transpose_out(torch.zeros(3, 8, 10)[:, :, :6], cpu, 3, 8, 6)
    for bad, frames in ((torch.zeros(6, 8), 1), (torch.zeros(8, 12)[:, ::2], 1), (torch.zeros(8, 6, dtype=torch.float64), 1),
                        (torch.zeros(8, 6, device="meta"), 1), (torch.zeros(8, 6), 3), (torch.zeros(2, 8, 6), 3),
                        (torch.zeros(3, 9, 6)[:, :8], 3), (torch.zeros(3, 6, 8).transpose(1, 2), 3), (torch.zeros(8, 5), 1)):
        with pytest.raises(CofiError, match="transpose"):
            ops._transpose_out(bad, cpu, frames, 8, 6)
