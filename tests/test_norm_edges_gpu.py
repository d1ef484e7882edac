"""The kernels of csrc/norm.hip at the shapes where they change path, against the float64 references of tests/norm_refs.py: LayerNorm at
every register count of a lane (C = 4 ... 2048) and every fill of a four-row workgroup, in all its activation / residual forms; the
GroupNorm statistics in both branches (column tiles, one workgroup per group), with a half-empty tile, more than 64 row slabs, stacked
frames and the fp64 `exact` path on offset data; the apply kernel with idle threads (C = 12, 20, 36), a second column pass (C = 1028), the
grid cap, every residual form, and its row_pos flag pinned at row sums of exactly zero; the fold of ColStats partials inside the kernel and
by the finalize launch; the column / row glue, the transposes and the second grid-stride trip of the sine embedding.
Every case goes through cofii2p_amd.ops, runs twice (the kernels have a fixed summation order: identical bits), and where an operand is
a view it is the column block at offset 4 of a wider buffer filled with 7.0, which the call must leave untouched around its output.

What runs what:
  layer_norm_act, layer_norm(relu, res), C = 4 ... 2048, strided operands    test_layer_norm_register_counts_and_row_fills, _offset_rows
  group branch at cpg 96 / 128 / 256, groups == 1, half-empty tile, exact    test_group_stats_both_branches
  more than 64 row slabs                                                     test_group_stats_more_than_64_row_slabs
  COFI_EUNSUPPORTED for cpg 3, 6, 12, 48                                     test_group_stats_refusals
  apply at C = 12, 20, 36, 1028, Mf = 1                                      test_group_norm_apply_widths_and_row_counts
  residual forms, gamma=None with a residual, slope 1                        test_group_norm_apply_forms
  the cap of 2048 workgroups                                                 test_group_norm_apply_grid_cap
  row_pos at a sum of exactly 0 / on every row                               test_row_pos_at_exactly_zero, test_row_pos_random_rows
  the in-kernel fold and cofi_norm_finalize                                  test_group_norm_apply_from_colstats
  col_inv_norm, l2norm_rows(2), col_mean at edge widths                      test_col_inv_norm_edges, test_l2norm_rows_edges, test_col_mean_edges
  pos_sine's second grid-stride trip                                         test_pos_sine_second_grid_stride_trip
  transpose(frames > 1), transpose(out=view), transpose_pair                 test_transpose_stacked_frames, _into_a_view, test_transpose_pair_mixed_halves
  host validation (ld >= C, 16-byte alignment, operand shapes)               test_norm_entry_points_refuse_operands_they_would_misread, ...
Needs a real MI355X:  python -m pytest tests/test_norm_edges_gpu.py -m gpu"""
import itertools

import numpy as np
import pytest
import torch

import norm_refs as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENT = 7.0
EPS = float(np.float32(1e-5))      # the kernels receive eps as a float: the references use the same number


@pytest.fixture(scope="module")
def ops():
    from cofii2p_amd import ops as _ops

    assert torch.cuda.is_available()
    saved, _ops.GEMM_MODE = _ops.GEMM_MODE, "f32"      # gemm_colstats(x, eye) is then exact
    yield _ops
    _ops.GEMM_MODE = saved


@pytest.fixture(scope="module")
def CofiError():
    from cofii2p_amd._lib import CofiError as E

    return E


def gen(seed):
    return torch.Generator().manual_seed(seed)


def G(t, dtype=None):
    return (t if dtype is None else t.to(dtype)).to(DEV)


def wide_of(t, off=4, pad=8):
    """(column block at `off` of a wider sentinel-filled device buffer that holds t, the buffer)"""
    M, C = t.shape
    W = (off + C + pad + 3) // 4 * 4
    wide = torch.full((M, W), SENT, device=DEV)
    wide[:, off:off + C] = t.to(DEV)
    return wide[:, off:off + C], wide


def place(t, strided, off=4):
    return wide_of(t, off)[0] if strided else G(t).contiguous()


def dest(M, C, strided, off=4):
    """-> (out operand, its buffer): sentinel everywhere, so that a row or column the kernel skips shows as 7.0 too"""
    if not strided:
        o = torch.full((M, C), SENT, device=DEV)
        return o, o
    return wide_of(torch.full((M, C), SENT), off)


def untouched(buf, out, off=4):
    """the sentinel columns around a view destination are still 7.0"""
    if buf is out:
        return
    C = out.shape[1]
    assert bool((buf[:, :off] == SENT).all()) and bool((buf[:, off + C:] == SENT).all()), "the kernel wrote outside its column block"


def all_sentinel(buf):
    assert bool((buf == SENT).all()), "a refused call wrote to its output"


def twice(run):
    """run() -> tensor or tuple of tensors, from fresh destinations: two runs, identical bits"""
    a, b = run(), run()
    for x, y in zip(a if isinstance(a, tuple) else (a,), b if isinstance(b, tuple) else (b,)):
        assert torch.equal(x, y), "two runs of the same call differ"
    return a


def close(got, ref, tol, what=""):
    np.testing.assert_allclose(got.detach().double().cpu().numpy(), ref.detach().double().cpu().numpy(), rtol=tol, atol=tol, err_msg=str(what))


def max_err(got, ref):
    return float((got.detach().double().cpu() - ref).abs().max())


# ====================================================================================================================== LayerNorm
LN_C = [4, 8, 252, 256, 260, 1028, 2044, 2048]
LN_M = [1, 3, 4, 5, 37]
# (function, keyword arguments, (slope, has res, res_first) of the reference)
LN_FORMS = ([("layer_norm", dict(relu=relu), (0.0 if relu else 1.0, res, False), res) for relu in (False, True) for res in (False, True)]
            + [("layer_norm_act", dict(slope=s, **({} if rf is None else {"res_first": rf})), (s, rf is not None, bool(rf)), rf is not None)
               for s in (0.0, 0.1, 1.0) for rf in (None, True, False)])


def ln_call(ops, form, x, ga, be, r, strided):
    """one LayerNorm call in the given layout -> (result, destination buffer)"""
    fn, kw, _, has_res = form
    M, C = x.shape
    out, buf = dest(M, C, strided)
    y = getattr(ops, fn)(place(x, strided), G(ga), G(be), res=place(r, strided) if has_res else None, out=out, **kw)
    assert y is out
    untouched(buf, out)
    return y


def ln_ref(form, x, ga, be, r):
    slope, has_res, res_first = form[2]
    return R.layer_norm_act(x, ga, be, EPS, slope, r if has_res else None, res_first)


def ln_two_pass_f32(form, x, ga, be, r):
    """the yardstick on offset rows: (x - mean(x)) / sqrt(mean((x - mean)^2) + eps) in fp32 torch on the CPU, then the form's affine,
    residual and activation in fp32 as well"""
    slope, has_res, res_first = form[2]
    mean = x.mean(1, keepdim=True)
    d = x - mean
    y = d / torch.sqrt((d * d).mean(1, keepdim=True) + EPS) * ga + be
    if has_res and res_first:
        y = y + r
    y = torch.where(y >= 0, y, y * slope)
    if has_res and not res_first:
        y = y + r
    return y


@pytest.mark.parametrize("C", LN_C)
def test_layer_norm_register_counts_and_row_fills(ops, C):
    """randn * 3 + 1 rows, one of them replaced by the constant 0.5: there every partial sum is exact, mean = 0.5, the centred row is 0
    and the output must be the fp32 value of act(beta (+ res)) (+ res) exactly."""
    g = gen(C)
    ga, be = torch.randn(C, generator=g), torch.randn(C, generator=g)
    for M in LN_M:
        x, r = torch.randn(M, C, generator=g) * 3 + 1, torch.randn(M, C, generator=g)
        k = M // 2
        x[k] = 0.5
        for form, strided in itertools.product(LN_FORMS, (False, True)):
            y = twice(lambda: ln_call(ops, form, x, ga, be, r, strided))
            close(y, ln_ref(form, x, ga, be, r), 2e-5, (form[:2], M, strided))
            slope, has_res, res_first = form[2]
            e = be + r[k] if has_res and res_first else be.clone()
            e = torch.where(e >= 0, e, e * slope)
            if has_res and not res_first:
                e = e + r[k]
            assert torch.equal(y[k].cpu(), e), ("constant row", form[:2], M, strided)


@pytest.mark.parametrize("C", LN_C)
def test_layer_norm_offset_rows(ops, C):
    """Rows of mean 100 and std 1.  The kernel is two-pass (mean, then centred squares), so it must stay within 4x the error of the same
    two-pass expression evaluated in fp32 by torch on the CPU ON THE SAME ROWS (the wave reduction orders the sums differently).  One
    or a few short rows can come out exact on the CPU by luck, so the yardstick has a floor: one ulp of the row mean (2^-17 at 100: the
    rounding of the fp32 sum and of its quotient) as it reaches the output, times the largest rstd |gamma| of the rows.
    Measured on an MI355X, largest absolute error over all forms and row counts against the float64 reference, kernel / CPU two-pass
    over 37 rows (outputs scaled by |gamma| up to 3.5):  C = 4: 1.7e-5 / 3.3e-5,  8: 1.5e-5 / 2.3e-5,  252: 2.5e-5 / 4.6e-5,
    256: 2.3e-5 / 4.5e-5,  260: 4.0e-5 / 4.8e-5,  1028: 3.7e-5 / 2.7e-5,  2044: 3.7e-5 / 3.6e-5,  2048: 3.3e-5 / 4.6e-5."""
    g = gen(1000 + C)
    ga, be = torch.randn(C, generator=g), torch.randn(C, generator=g)
    pool, rpool = torch.randn(37, C, generator=g) + 100, torch.randn(37, C, generator=g)
    rstd = 1.0 / torch.sqrt(pool.double().var(1, unbiased=False) + EPS)
    worst_k = worst_y = 0.0
    for form in LN_FORMS:
        ref = ln_ref(form, pool, ga, be, rpool)
        cpu_err = (ln_two_pass_f32(form, pool, ga, be, rpool).double() - ref).abs().amax(1)      # per row
        for M, strided in itertools.product(LN_M, (False, True)):
            yard = max(float(cpu_err[:M].max()), 2.0 ** -17 * float(rstd[:M].max()) * float(ga.abs().max()))
            y = twice(lambda: ln_call(ops, form, pool[:M], ga, be, rpool[:M], strided))
            err = max_err(y, ref[:M])
            worst_k, worst_y = max(worst_k, err), max(worst_y, yard)
            print("layer norm offset rows C=%d %s M=%d strided=%d: kernel %.3g, fp32 two-pass on the CPU %.3g" % (C, form[:2], M, strided, err, yard))
            assert err <= 4 * yard, (form[:2], M, strided, err, yard)
    print("layer norm offset rows C=%d: worst kernel %.3g, worst yardstick %.3g" % (C, worst_k, worst_y))


@pytest.mark.parametrize("C", [2052, 6])
def test_layer_norm_refuses_widths_it_cannot_hold(ops, CofiError, C):
    x, v = torch.zeros(3, C, device=DEV), torch.ones(C, device=DEV)
    for call in (lambda o: ops.layer_norm(x, v, v, out=o), lambda o: ops.layer_norm_act(x, v, v, out=o)):
        out = torch.full((3, C), SENT, device=DEV)
        with pytest.raises(CofiError):
            call(out)
        all_sentinel(out)


# ====================================================================================================================== group_stats
GS_TILE = [(4, 1), (8, 1), (96, 24), (32, 32)]                  # column-tile branch (cpg < 64); (96, 24): half-empty last tile, cpg 4
GS_GROUP = [(192, 3), (192, 2), (256, 2), (256, 1)]             # one workgroup per group: cpg 64, 96, 128, 256
GS_MF = [1, 3, 63, 64, 65, 130]


def stats_close(st, x, groups, frames, tol, what):
    """mean and rstd within `tol` RELATIVE of the float64 reference"""
    mean, rstd = R.group_stats(x, groups, EPS, frames)
    st = st.detach().double().cpu().reshape(frames, groups, 2)
    for name, got, ref in (("mean", st[..., 0], mean), ("rstd", st[..., 1], rstd)):
        rel = float(((got - ref).abs() / ref.abs()).max())
        assert rel <= tol, (what, name, rel)
    return st


@pytest.mark.parametrize("exact", [False, True])
@pytest.mark.parametrize("C,groups", GS_TILE + GS_GROUP)
def test_group_stats_both_branches(ops, C, groups, exact):
    """serving path (the sum of a thread's own values in fp32 - 16 rows of one column, or of cpg / 64 columns in the group branch: at
    most 64 values at the widths here - and everything above in fp64): 5e-6 relative at mean 0.7 / std 2, from 64 * 2^-24 * E[x^2] / var;
    exact path (every sum fp64): the correctly rounded value with two bits of margin, 2^-22, also at mean 1000 / std 1.
    What this found: the serving path squared in fp32.  A group of one value (C = groups = 32, one row) has variance 0, but came out
    with var = fl(x^2) - x^2 ~ 1e-7 next to eps = 1e-5: rstd 0.9 % off.  The kernel now forms and sums the squares in fp64 on both paths."""
    g = gen(C * 7 + groups)
    for Mf, frames, strided in itertools.product(GS_MF, (1, 3), (False, True)):
        if strided and Mf not in (3, 65):
            continue
        kinds = [torch.randn(frames * Mf, C, generator=g) * 2 + 0.7]
        if exact:
            kinds.append(torch.randn(frames * Mf, C, generator=g) + 1000)
        for i, x in enumerate(kinds):
            xd = place(x, strided, off=3)          # the statistics kernel reads scalars: any column offset is legal
            st = twice(lambda: ops.group_stats(xd, groups, frames=frames, exact=exact))
            assert st.shape == ((groups, 2) if frames == 1 else (frames, groups, 2))
            stats_close(st, x, groups, frames, 2.0 ** -22 if exact else 5e-6, (Mf, frames, strided, i))


@pytest.mark.parametrize("exact", [False, True])
@pytest.mark.parametrize("groups", [1, 2, 8])
def test_group_stats_more_than_64_row_slabs(ops, groups, exact):
    """4100 rows = 65 slabs: lane 0 of the final kernel takes a second partial"""
    x = torch.randn(4100, 8, generator=gen(groups)) * 2 + 0.7
    st = twice(lambda: ops.group_stats(G(x), groups, exact=exact))
    stats_close(st, x, groups, 1, 2.0 ** -22 if exact else 5e-6, groups)
    x3 = torch.cat([x, x * 0.5 + 1, x - 2])
    st3 = twice(lambda: ops.group_stats(G(x3), groups, frames=3, exact=exact))
    stats_close(st3, x3, groups, 3, 2.0 ** -22 if exact else 5e-6, groups)
    assert torch.equal(st3[0], st)


@pytest.mark.parametrize("exact", [False, True])
def test_group_stats_refusals(ops, CofiError, exact):
    for cpg in (3, 6, 12, 48):       # below one wave a group is a power-of-two run of lanes
        with pytest.raises(CofiError, match="UNSUPPORTED"):
            ops.group_stats(torch.zeros(5, 4 * cpg, device=DEV), 4, exact=exact)
    for C, groups in ((10, 4), (64, 3), (4, 8)):
        with pytest.raises(CofiError):
            ops.group_stats(torch.zeros(5, C, device=DEV), groups, exact=exact)


# ====================================================================================================================== group_norm_apply
def ref_stats(x, groups, frames):
    """float64 statistics rounded to the fp32 (frames, groups, 2) tensor the kernel is handed; the reference apply then starts from these
    very numbers, so that the comparison judges the apply kernel alone (and groups of any width can be used)"""
    mean, rstd = R.group_stats(x, groups, EPS, frames)
    st = torch.stack([mean, rstd], -1).float()
    return st[0] if frames == 1 else st


RES_FORMS = ["none", "res", "res+stats", "res+stats+affine"]


def gn_case(ops, x, r, groups, frames, affine, res_form, slope, strided, g, tol=2e-5, want_row_pos=False):
    M, C = x.shape
    ga, be = (1 + 0.1 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)) if affine else (None, None)
    rga, rbe = (0.3 * torch.randn(C, generator=g), 1 + 0.1 * torch.randn(C, generator=g)) if res_form == "res+stats+affine" else (None, None)
    st = ref_stats(x, groups, frames)
    rst = ref_stats(r, groups, frames) if res_form.startswith("res+stats") else None
    res = r if res_form != "none" else None
    dv = lambda t: None if t is None else G(t)

    def run():
        out, buf = dest(M, C, strided)
        y = ops.group_norm_apply(place(x, strided), G(st), dv(ga), dv(be), slope=slope, res=None if res is None else place(res, strided),
                                 res_stats=dv(rst), res_gamma=dv(rga), res_beta=dv(rbe), out=out, frames=frames, want_row_pos=want_row_pos)
        assert y is out
        untouched(buf, out)
        return (y, y.cofi_row_pos) if want_row_pos else y

    got = twice(run)
    ref = R.group_norm_apply(x, st, ga, be, slope, res, rst, rga, rbe, frames)
    what = (M, C, groups, frames, affine, res_form, slope, strided)
    if M // frames * (C // groups) > 1:
        close(got[0] if want_row_pos else got, ref, tol, what)
    else:
        # A group of ONE value: variance 0, rstd = eps^-1/2 = 316, and the exact result is act(beta + residual term).  The kernel
        # evaluates x * sc + sh with sc = rstd gamma, sh = beta - mean rstd gamma (the form it shares with the normalising GEMM loader):
        # two terms of size P = |x| rstd |gamma| that cancel.  Roundings of that size: sc, mean * rstd, (mean rstd) * gamma, the
        # subtraction in sh, and x * sc where it is not fused into the final fma -> 5 * 2^-24 P on top of the benign tolerance, per
        # normalised operand.  (Benign groups have rstd ~ 0.5, where this term is below 1e-6.)
        cols = lambda s, v: s.reshape(frames, groups, 2)[..., 1].double().repeat_interleave(M // frames, 0) * (1.0 if v is None else v.double().abs())
        extra = x.double().abs() * cols(st, ga)
        if rst is not None:
            extra = extra + r.double().abs() * cols(rst, rga)
        err = ((got[0] if want_row_pos else got).detach().double().cpu() - ref).abs()
        assert bool((err <= tol + tol * ref.abs() + 5 * 2.0 ** -24 * extra).all()), (what, float(err.max()))
    return got, ref


@pytest.mark.parametrize("C", [4, 12, 20, 36, 64, 256, 1024, 1028, 2048])
def test_group_norm_apply_widths_and_row_counts(ops, C):
    """threads per row 1, 3, 5, 9 (idle threads in the block), 16, 64, 256, 256 + one thread's second pass, 256 x 2"""
    g = gen(C)
    for Mf, frames in itertools.product((1, 5, 257), (1, 3)):
        x, r = torch.randn(frames * Mf, C, generator=g) * 2 + 0.7, torch.randn(frames * Mf, C, generator=g)
        for i, groups in enumerate((1, C // 4, C)):
            gn_case(ops, x, r, groups, frames, affine=True, res_form=RES_FORMS[(i + Mf) % 4], slope=0.1, strided=bool((i + frames) & 1), g=g)


@pytest.mark.parametrize("C", [36, 1028])
def test_group_norm_apply_forms(ops, C):
    """every residual form x affine or not (gamma=None with a residual included) x slope 0 / 0.1 / 1 x layout x frames x group width"""
    g = gen(C + 1)
    for frames in (1, 3):
        x, r = torch.randn(frames * 5, C, generator=g) * 2 + 0.7, torch.randn(frames * 5, C, generator=g) * 1.5 - 0.4
        for affine, res_form, slope, strided, groups in itertools.product((False, True), RES_FORMS, (0.0, 0.1, 1.0), (False, True), (1, C // 4, C)):
            gn_case(ops, x, r, groups, frames, affine, res_form, slope, strided, g)


def test_group_norm_apply_grid_cap(ops):
    """8197 rows of 1024: 2050 workgroups wanted, 2048 launched; rows from 8192 on are the second trip of the row loop, whose loads for
    the rows past the end are clamped to the last row"""
    g = gen(8197)
    x, r = torch.randn(8197, 1024, generator=g) * 2 + 0.7, torch.randn(8197, 1024, generator=g)
    gn_case(ops, x, r, 32, 1, affine=True, res_form="res+stats+affine", slope=0.1, strided=False, g=g)


ROW_POS_C = [4, 8, 16, 32, 64, 128, 256]


@pytest.mark.parametrize("C", ROW_POS_C)
def test_row_pos_random_rows(ops, C):
    """slope 1, so both signs reach the sum.  The flag is the sign of the fp32 tree sum of the returned y (norm_refs.row_sum_tree_f32) on
    every row, and the sign of the float64 row sum wherever |s| > C 2^-24 sum_c |y[m, c]|, the worst case of any summation order; the
    inputs are chosen so that the float64 reference alone leaves at most 1 % of the rows inside that band."""
    g = gen(C + 2)
    frames, Mf = 3, 259
    x, r = torch.randn(frames * Mf, C, generator=g) * 2 + 0.7, torch.randn(frames * Mf, C, generator=g)
    (y, rp), ref = gn_case(ops, x, r, max(1, C // 4), frames, affine=True, res_form="res", slope=1.0, strided=(C % 3 == 1), g=g, want_row_pos=True)
    assert rp.dtype == torch.uint8 and rp.shape == (frames * Mf,)
    rp = rp.cpu().bool()
    assert torch.equal(rp, R.row_sum_tree_f32(y) > 0), "row_pos is not the sign of the kernel's own fp32 row sum"
    band = lambda v: v.sum(1).abs() <= C * 2.0 ** -24 * v.abs().sum(1)
    assert int(band(ref).sum()) <= 0.01 * ref.shape[0], "the inputs leave too many rows undecided in float64"
    firm = ~band(y.double().cpu()) & ~band(ref)
    assert int((~firm).sum()) <= 0.01 * ref.shape[0]
    assert torch.equal(rp[firm], (ref.sum(1) > 0)[firm])


@pytest.mark.parametrize("C", ROW_POS_C)
def test_row_pos_at_exactly_zero(ops, C):
    """statistics (mean 0, rstd 1) without affine make y = leaky(x) exactly.  The kernel says `> 0`: a row of zeros (slope 0 on an
    all-negative row) and a row whose tree sum cancels exactly (slope 1, +a, -a in adjacent columns) are NOT positive, the all-negative
    row with a single +1e-30 is.  The pinned rows include the last row of each frame."""
    g = gen(C + 3)
    frames, Mf, groups = 2, 5, max(1, C // 4)
    M = frames * Mf
    st = torch.tensor([0.0, 1.0]).repeat(frames, groups, 1)
    neg = -(torch.rand(M, C, generator=g) + 0.5)
    # slope 0
    x = torch.randn(M, C, generator=g)
    x[1], x[Mf - 1], x[M - 1] = neg[1], neg[Mf - 1], neg[M - 1]
    x[Mf], x[M - 2] = neg[Mf], neg[M - 2]
    x[Mf, C // 2], x[M - 2, C - 1] = 1e-30, 1e-30
    for strided in (False, True):
        def run():
            out, buf = dest(M, C, strided)
            y = ops.group_norm_apply(place(x, strided), G(st), slope=0.0, out=out, frames=frames, want_row_pos=True)
            untouched(buf, out)
            return y, y.cofi_row_pos
        y, rp = twice(run)
        assert torch.equal(y.cpu(), torch.relu(x))
        rp = rp.cpu()
        assert [int(rp[m]) for m in (1, Mf - 1, M - 1)] == [0, 0, 0], "a row of zeros is flagged positive"
        assert [int(rp[m]) for m in (Mf, M - 2)] == [1, 1], "a row sum of 1e-30 is not flagged positive"
        assert torch.equal(rp.bool(), R.row_sum_tree_f32(y) > 0)
    # slope 1: +a, -a in adjacent columns: (v0 + v1) and (v2 + v3) are 0 in every chunk
    a = torch.randn(M, C // 2, generator=g) * 3
    z = torch.stack([a, -a], -1).reshape(M, C)
    x = torch.randn(M, C, generator=g) - 0.1
    for m in (0, Mf - 1, M - 1):
        x[m] = z[m]
    assert bool((R.row_sum_tree_f32(x)[[0, Mf - 1, M - 1]] == 0).all())
    y, rp = twice(lambda: (lambda o: (o, o.cofi_row_pos))(ops.group_norm_apply(G(x), G(st), slope=1.0, frames=frames, want_row_pos=True)))
    assert torch.equal(y.cpu(), x)
    rp = rp.cpu()
    assert [int(rp[m]) for m in (0, Mf - 1, M - 1)] == [0, 0, 0], "a row that sums to exactly 0 is flagged positive"
    assert torch.equal(rp.bool(), R.row_sum_tree_f32(y) > 0)


@pytest.mark.parametrize("C", [12, 512])
def test_row_pos_is_not_offered_where_a_row_is_not_a_lane_group(ops, C):
    x = torch.randn(5, C, generator=gen(C))
    y = ops.group_norm_apply(G(x), G(ref_stats(x, C // 4, 1)), want_row_pos=True)
    assert not hasattr(y, "cofi_row_pos")
    close(y, R.group_norm_apply(x, ref_stats(x, C // 4, 1)), 2e-5)


# ====================================================================================================================== from ColStats
@pytest.mark.parametrize("finalize_min_frames", [1, 0])
@pytest.mark.parametrize("frames,Mf,C,groups,own_res", [
    (1, 5, 4, 1, False), (1, 5, 4, 2, True), (1, 5, 4, 4, False),          # minimal table, one slab
    (1, 64 * 128 + 1, 64, 32, False),                                       # second trip of the slab loop at 8 phases
    (1, 64 * 16 + 1, 1024, 32, False), (1, 64 * 16 + 1, 1024, 1024, False),   # two column passes, second slab trip
    (3, 128, 64, 32, False)])
def test_group_norm_apply_from_colstats(ops, monkeypatch, finalize_min_frames, frames, Mf, C, groups, own_res):
    """statistics partials of gemm_colstats(x, eye(C)) (exact in the f32 mode) folded by every workgroup of the apply kernel
    (FINALIZE_MIN_FRAMES = 0) or once by cofi_norm_finalize (= 1); the reference starts from the GEMM's own output"""
    monkeypatch.setattr(ops, "FINALIZE_MIN_FRAMES", finalize_min_frames)
    g = gen(Mf + C + groups)
    M = frames * Mf
    x, r = torch.randn(M, C, generator=g) * 2 + 0.7, torch.randn(M, C, generator=g) * 1.5 - 0.4
    ga, be = 1 + 0.1 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)
    eye = torch.eye(C, device=DEV)
    y, part = ops.gemm_colstats(G(x), eye)
    assert torch.equal(y.cpu(), x)
    yr, rpart = ops.gemm_colstats(G(r), eye)
    want_rp = C <= 256

    def run():
        st = ops.ColStats(part, M, groups, frames, eps=EPS)
        assert st.fusable()
        rst = ops.ColStats(rpart, M, groups, frames, eps=EPS) if own_res else None
        out = ops.group_norm_apply(y, st, G(ga), G(be), slope=0.1, res=yr, res_stats=rst, res_gamma=G(be) if own_res else None,
                                   res_beta=G(ga) if own_res else None, frames=frames, want_row_pos=want_rp)
        return (out, out.cofi_row_pos) if want_rp else out

    got = twice(run)
    out = got[0] if want_rp else got
    yc = y.cpu()
    ref = R.group_norm_apply(yc, R.group_stats(yc, groups, EPS, frames), ga, be, 0.1, r, R.group_stats(r, groups, EPS, frames) if own_res else None,
                             be if own_res else None, ga if own_res else None, frames)
    close(out, ref, 2e-5)
    if want_rp:
        assert torch.equal(got[1].cpu().bool(), R.row_sum_tree_f32(out) > 0)


# ====================================================================================================================== column / row glue
@pytest.mark.parametrize("C", [4, 16, 20, 132])
def test_col_inv_norm_edges(ops, C):
    g = gen(C)
    floor = (torch.tensor(1.0) / torch.tensor(1e-12)).item()           # fp32 1 / fp32 1e-12
    for M, strided in itertools.product((1, 63, 64, 65, 1281), (False, True)):
        x = torch.randn(M, C, generator=g)
        x[:, C - 1] = 0
        got = twice(lambda: ops.col_inv_norm(place(x, strided)))
        assert got.shape == (C,)
        close(got[:C - 1], R.col_inv_norm(x)[:C - 1], 1e-5, (M, strided))
        assert float(got[C - 1]) == floor, "an all-zero column must give 1 / eps exactly"


def test_col_inv_norm_refuses_a_misaligned_view(ops, CofiError):
    wide = torch.randn(5, 16, device=DEV)
    with pytest.raises(CofiError):
        ops.col_inv_norm(wide[:, 2:10])


@pytest.mark.parametrize("C", [64, 100])
def test_col_inv_norm_from_colpart_edges(ops, C):
    """the first C of 128 partial columns; M = 64: one slab, three of the four slab phases empty"""
    g = gen(C)
    eye = torch.eye(128, device=DEV)
    for M, frames in ((64, 1), (321, 1), (128, 2)):
        x = torch.randn(M, 128, generator=g)
        y, part = ops.gemm_colstats(G(x), eye)
        got = twice(lambda: ops.col_inv_norm_from_colpart(part, M, C, frames=frames))
        assert got.shape == ((C,) if frames == 1 else (frames, C))
        ref = torch.stack([R.col_inv_norm(f[:, :C]) for f in x.reshape(frames, M // frames, 128)])
        close(got.reshape(frames, C), ref, 1e-5, (M, frames))


L2_KINDS = {"randn": 1.0, "zero": 0.0, "tiny": 1e-12, "huge": 1e15}      # squares of 1e-12 and 1e15 are normal and finite in fp32


@pytest.mark.parametrize("C", [1, 3, 63, 64, 65, 130])
def test_l2norm_rows_edges(ops, C):
    g = gen(C)
    five = torch.randn(5, C, generator=g)
    for m, k in enumerate(("randn", "zero", "tiny", "huge")):
        five[m] *= L2_KINDS[k]
    inputs = [five] + [torch.randn(1, C, generator=g) * s for s in L2_KINDS.values()]
    for x, strided in itertools.product(inputs, (False, True)):
        M = x.shape[0]
        ref = R.l2norm_rows(x)
        xd = place(x, strided)

        def plain():
            out, buf = dest(M, C, strided)
            y = ops.l2norm_rows(xd, out=out)
            untouched(buf, out)
            return y

        def transposed():       # out (C, M), as rows of a wider buffer when strided: ldy > M
            out, buf = dest(C, M, strided)
            y = ops.l2norm_rows(xd, out=out, transpose=True)
            untouched(buf, out)
            return y

        def both():
            (o1, b1), (o2, b2) = dest(M, C, strided), dest(M, C, not strided)
            ops.l2norm_rows2(xd, o1, o2)
            untouched(b1, o1), untouched(b2, o2)
            return o1, o2

        y, yt, (y1, y2) = twice(plain), twice(transposed), twice(both)
        close(y, ref, 1e-6, (M, strided))
        assert torch.equal(yt, y.t()) and torch.equal(y1, y) and torch.equal(y2, y)
        if M == 5:
            assert torch.equal(y[1].cpu(), torch.zeros(C)), "a zero row must stay exactly zero"
        assert bool(torch.isfinite(y).all())


@pytest.mark.parametrize("C", [1, 63, 65, 130])
def test_col_mean_edges(ops, C):
    g = gen(C)
    for Mf, frames, strided in itertools.product((1, 3, 4, 5, 160), (1, 3), (False, True)):
        x = torch.randn(frames * Mf, C, generator=g)
        got = twice(lambda: ops.col_mean(place(x, strided), frames))
        assert got.shape == (frames, C)
        close(got, R.col_mean(x, frames), 1e-6, (Mf, frames, strided))


@pytest.mark.parametrize("Mf,C", [(68, 64), (33, 5)])
def test_transpose_stacked_frames(ops, Mf, C):
    """(68, 64): the float4 kernel with a partial row tile; (33, 5): the scalar kernel"""
    x = torch.randn(3 * Mf, C, generator=gen(Mf))
    for strided in (False, True):
        got = twice(lambda: ops.transpose(place(x, strided), frames=3))
        assert got.shape == (3, C, Mf)
        assert torch.equal(got.cpu(), x.reshape(3, Mf, C).transpose(1, 2))


@pytest.mark.parametrize("M,C", [(68, 64), (33, 5)])
def test_transpose_into_a_view(ops, M, C):
    x = torch.randn(M, C, generator=gen(M + 1))

    def run():
        out, buf = dest(C, M, True)       # ldy > M
        y = ops.transpose(G(x), out=out)
        assert y is out
        untouched(buf, out)
        return y

    assert torch.equal(twice(run).cpu(), x.t())


@pytest.mark.parametrize("M,C1,C2", [(68, 64, 6), (70, 64, 6)])
def test_transpose_pair_mixed_halves(ops, M, C1, C2):
    """M = 68: a float4 half and a scalar half in one launch; M = 70: both halves scalar"""
    g = gen(M)
    a, b = torch.randn(M, C1, generator=g), torch.randn(M, C2, generator=g)
    for strided in (False, True):
        at, bt = twice(lambda: ops.transpose_pair(place(a, strided), place(b, strided)))
        assert torch.equal(at.cpu(), a.t()) and torch.equal(bt.cpu(), b.t())


@pytest.mark.parametrize("kind", ["grid", "xyz"])
def test_pos_sine_second_grid_stride_trip(ops, kind):
    """T = 4100 tokens x 128 channels > 2048 x 256 threads.  The angle is formed in fp32 from one multiplication and one division by an
    fp32 dim_t (three roundings with the table's own), sinf / cosf add an ulp: |ang|max 2^-22 + 2^-22 absolute."""
    g = gen(len(kind))
    T = 4100
    if kind == "grid":
        coords = torch.stack([torch.randint(0, 64, (T,), generator=g), torch.randint(0, 20, (T,), generator=g)], 1).to(torch.int32)
    else:
        coords = (torch.rand(T, 3, generator=g) * 160 - 80).float()
        coords[0], coords[T - 1] = torch.tensor([80.0, -80.0, 0.0]), torch.tensor([-80.0, 80.0, 79.5])
    n_dim = coords.shape[1]
    ref, amax = R.pos_sine(coords, 128)
    base = torch.randn(T, 128, generator=g)

    def run(accumulate):
        out = torch.full((T, 160), SENT, device=DEV)
        out[:, :128] = G(base)
        y = ops.pos_sine(G(coords), out, accumulate=accumulate)
        assert y is out and bool((out[:, 128:] == SENT).all()), "columns 128 ... 159 belong to the caller"
        return out[:, :128]

    plain, acc = twice(lambda: run(False)).cpu(), twice(lambda: run(True)).cpu()
    err = max_err(plain, ref)
    print("pos_sine %s: max error %.3g at |ang| <= %.4g, bound %.3g" % (kind, err, amax, amax * 2.0 ** -22 + 2.0 ** -22))
    assert err <= amax * 2.0 ** -22 + 2.0 ** -22
    assert torch.equal(acc, base + plain), "accumulate=True must add exactly what accumulate=False writes"
    if n_dim == 3:      # 3 x 42 = 126 channels carry the embedding
        assert torch.equal(plain[:, 126:], torch.zeros(T, 2)) and torch.equal(acc[:, 126:], base[:, 126:])


# ====================================================================================================================== refusals
# No operand below is short: each is as large as the call's shapes ask for, or is the head of a larger buffer that holds every element
# a launch with these arguments would touch (rows, frames and groups included).  A missing check therefore shows as a failed assertion,
# never as an access outside an allocation.  Operands that are plainly too short are refused on the CPU only (test_norm_refs_cpu.py).
def _norm_calls(ops):
    """name -> call(x, gamma, beta, res, out) of the four entry points that read and write float4 rows"""
    def from_colstats(x, ga, be, res, out):
        M, C = x.shape
        _, part = ops.gemm_colstats(torch.zeros(M, C, device=DEV), torch.eye(C, device=DEV))
        return ops.group_norm_apply(x, ops.ColStats(part, M, C // 4, 1), ga, be, res=res, out=out)

    return {
        "layer_norm": lambda x, ga, be, res, out: ops.layer_norm(x, ga, be, res=res, out=out),
        "layer_norm_act": lambda x, ga, be, res, out: ops.layer_norm_act(x, ga, be, slope=0.1, res=res, out=out),
        "group_norm_apply": lambda x, ga, be, res, out: ops.group_norm_apply(x, torch.tensor([[0.0, 1.0]] * (x.shape[1] // 4), device=DEV), ga, be,
                                                                              res=res, out=out),
        "group_norm_apply/ColStats": from_colstats,
    }


@pytest.mark.parametrize("entry", ["layer_norm", "layer_norm_act", "group_norm_apply", "group_norm_apply/ColStats"])
def test_norm_entry_points_refuse_operands_they_would_misread(ops, CofiError, entry):
    call = _norm_calls(ops)[entry]
    M, C = 6, 16
    big = torch.randn(4096, device=DEV)                       # every view below stays far inside it
    x, res = big[:M * C].reshape(M, C), big[1024:1024 + M * C].reshape(M, C)
    ga, be = torch.ones(C, device=DEV), torch.zeros(C, device=DEV)
    wide = big[2048:2048 + M * 32].reshape(M, 32)
    cases = {
        "gamma too long": dict(ga=torch.ones(C + 4, device=DEV)),
        "beta too long": dict(be=torch.zeros(2 * C, device=DEV)),
        "res with more columns": dict(res=big[1024:1024 + M * (C + 4)].reshape(M, C + 4)),
        "res with more rows": dict(res=big[1024:1024 + (M + 2) * C].reshape(M + 2, C)),
        "x misaligned": dict(x=wide[:, 2:2 + C]),
        "res misaligned": dict(res=wide[:, 6:6 + C]),
        "ldx < C": dict(x=big.as_strided((M, C), (C - 4, 1))),
        "ldr < C": dict(res=big.as_strided((M, C), (C - 8, 1), 1024)),
    }
    for what, kw in cases.items():
        out = torch.full((M, C), SENT, device=DEV)
        args = dict(x=x, ga=ga, be=be, res=res, out=out)
        args.update(kw)
        with pytest.raises(CofiError):
            call(args["x"], args["ga"], args["be"], args["res"], args["out"])
        all_sentinel(out)
    # destinations: a misaligned view, rows that overlap (ldy < C), a wrong shape
    obuf = torch.full((M, 32), SENT, device=DEV)
    flat = torch.full((M * C,), SENT, device=DEV)
    for what, out in (("out misaligned", obuf[:, 2:2 + C]), ("ldy < C", flat.as_strided((M, C), (C - 4, 1))), ("out too wide", obuf[:, 4:8 + C]),
                      ("out too short", obuf[:M - 1, 4:4 + C])):
        with pytest.raises(CofiError):
            call(x, ga, be, res, out)
        all_sentinel(obuf), all_sentinel(flat)
    if entry.startswith("layer_norm"):      # gamma / beta are read as float4 too
        gb = torch.ones(C + 4, device=DEV)
        for kw in (dict(ga=gb[1:C + 1]), dict(be=gb[3:C + 3])):
            out = torch.full((M, C), SENT, device=DEV)
            args = dict(ga=ga, be=be)
            args.update(kw)
            with pytest.raises(CofiError):
                call(x, args["ga"], args["be"], res, out)
            all_sentinel(out)
    # and the same operands, in order, are accepted
    out = torch.full((M, C), SENT, device=DEV)
    call(x, ga, be, res, out)
    assert not bool((out == SENT).any())


def test_group_norm_apply_refuses_statistics_of_another_shape(ops, CofiError):
    M, C = 6, 16
    x, res = torch.randn(M, C, device=DEV), torch.randn(M, C, device=DEV)
    # every statistics operand is the head of a 16-group buffer: no frame or group index the kernel could form from these arguments
    # (frames <= 3, groups <= 16) leaves it
    room = torch.tensor([[0.0, 1.0]] * 16, device=DEV)
    st = room[:4]
    bad = [dict(stats=st[:, :1]), dict(stats=room[:12].reshape(3, 4, 2)), dict(stats=room.double()[:4]), dict(stats=st, frames=2), dict(stats=room[:11]),
           dict(stats=st, res=res, res_stats=room[:8]), dict(stats=room[:8], res=res, res_stats=st),
           dict(stats=st, res=res, res_stats=st, res_gamma=torch.ones(C + 4, device=DEV), res_beta=torch.ones(C + 4, device=DEV))]
    for kw in bad:
        out = torch.full((M, C), SENT, device=DEV)
        with pytest.raises(CofiError):
            ops.group_norm_apply(x, kw.pop("stats"), out=out, **kw)
        all_sentinel(out)


def test_transpose_refuses_a_destination_of_another_shape(ops, CofiError):
    """each destination is a view of a buffer that holds every element a launch with these arguments would write: (8, 12) from the first
    case's 96 floats at ldy 8, ..., the two-frame destination is the head of a three-frame buffer"""
    x = torch.randn(12, 8, device=DEV)
    full = lambda *shape: torch.full(shape, SENT, device=DEV)
    for view, frames in ((lambda b: b, 1), (lambda b: b.reshape(8, 24)[:, :16:2], 1), (lambda b: b.reshape(3, 8, 8)[:, :, :4].transpose(1, 2), 3),
                         (lambda b: b.reshape(3, 8, 8)[:2, :, :4], 3), (lambda b: b.reshape(3, 16, 4)[:, :8], 3)):      # right shape, frames 16 rows apart
        buf = full(24, 8)
        with pytest.raises(CofiError):
            ops.transpose(x, out=view(buf), frames=frames)
        all_sentinel(buf)
